"""CPU: the single definitions the trainers and loss wrappers share — the count-to-Dice function, the relation between
``loss_values`` and ``loss_table`` (every closed form is written in ``loss_table`` alone), and the argparse flags of the two trainer
modules, which one builder produces.  The C ABI is routed through the emulator."""
from argparse import ArgumentParser

import pytest
import torch

from abi_emulator import Emulator, emulated
from capstone_amd import segloss
from feature_emulators import BoundaryEntries, MixupEntries


class E(BoundaryEntries, MixupEntries, Emulator):
    pass


@pytest.fixture()
def emu():
    with emulated(E(), plan_run=False) as e:
        yield e


def test_dice_from_counts_is_one_function():
    """(B, 3, C) counts = [intersection, predicted, true] per class: class 4 has no truth in sample 0, class 7 in no sample"""
    g = torch.Generator().manual_seed(2)
    true = torch.randint(5, 40, (3, 10), generator=g)
    pred = torch.randint(5, 40, (3, 10), generator=g)
    true[0, 4] = 0
    true[:, 7] = 0
    inter = torch.minimum(torch.minimum(true, pred), torch.randint(0, 40, (3, 10), generator=g))
    cnt = torch.stack([inter, pred, true], dim=1)
    assert cnt.shape == (3, 3, 10) and cnt.dtype == torch.int64
    mean, per_class = segloss.dice_metric(cnt)
    eng = segloss.SegLossEngine(torch.device("cpu"), 3, 64, 10)
    eng.cnt.copy_(cnt)
    e_mean, e_per_class = eng.dice_metric()
    assert torch.equal(mean, e_mean) and torch.equal(per_class, e_per_class)
    # the all-empty class scores 0 and leaves no NaN behind; the half-empty one is the mean over the samples that have it
    assert per_class.shape == (9,) and torch.isfinite(per_class).all() and torch.isfinite(mean) and per_class[6] == 0
    d = 2.0 * inter.float() / (true + pred).float()
    assert torch.equal(per_class[3], (d[1, 4] + d[2, 4]) / 2.0) and torch.equal(per_class[0], d[:, 1].sum() / 3.0)
    assert torch.equal(mean, per_class.mean())
    # the (B, 2, 3, C) pair counts of the mixup step: a side is a strided slice
    cnt2 = torch.stack([cnt, cnt.flip(0)], dim=1)
    for s, want in enumerate((cnt, cnt.flip(0))):
        got_mean, got_per = segloss.dice_metric(cnt2[:, s])
        want_mean, want_per = segloss.dice_metric(want.contiguous())
        assert not cnt2[:, s].is_contiguous() and torch.equal(got_mean, want_mean) and torch.equal(got_per, want_per)


@pytest.mark.parametrize("exclude_missing", [False, True])
@pytest.mark.parametrize("name", ["Dice", "GeneralizedDice", "Focal", "Boundary"])
def test_loss_value_is_the_weighted_sum_of_its_table(emu, name, exclude_missing):
    from capstone_amd.models.losses import _as_cl
    g = torch.Generator().manual_seed(7)
    logits = torch.randn(2, 10, 4, 4, 2, generator=g) * 2
    target = torch.randint(0, 10, (2, 4, 4, 2), generator=g)
    target[0][target[0] == 4] = 0                                  # a class without truth in one sample
    ind = None
    if exclude_missing:
        ind = torch.ones(2, 9)
        ind[1, 3] = 0
        ind[:, 6] = 0                                              # a class nobody annotates: the isinf branch of the weights
    eng = segloss.SegLossEngine(torch.device("cpu"), 2, 32, 10)
    eng.set_target(target)
    eng.set_dist_maps(torch.rand(2, 9, 4, 4, 2, generator=g) * 2 - 1)
    ptr, ld, _keep = _as_cl(logits)
    value = eng.loss_forward(ptr, ld, [name], exclude_missing, ind)[name]
    table = eng.loss_table(name)
    assert table.shape == ((2, 10) if name == "Focal" else (2, 9)) and table.dtype == torch.float32
    w = eng._w[name]
    if name in ("Dice", "GeneralizedDice"):                        # their gradient weights carry a zero background column
        assert w.shape == (2, 10) and not w[:, 0].any()
        w = w[:, 1:]
    assert w.shape == table.shape
    assert value.ndim == 0 and value.dtype == torch.float32 and torch.equal(value, (table * w).sum())
    if exclude_missing:
        fg = w[:, 1:] if name == "Focal" else w                    # (Focal's table has a background column in front)
        assert not fg[1, 3] and not fg[:, 6].any() and fg[0, 0] > 0
    else:
        assert torch.equal(w, torch.full_like(w, 1.0 / w.numel()))


def test_both_parsers_keep_the_reference_flags_and_defaults():
    from capstone_amd.training.base_trainer import BaseUNet2D
    from capstone_amd.training.mixup_trainer import MixupUNet2D
    from capstone_amd.volumetric.base_trainer import BaseUNet3D
    three_d = {"batch_size": 1, "transform_degree": 0, "filters": [64, 128, 256, 512, 1024], "use_res_units": False,
               "downsample": False, "lr": 0.001, "loss_fx": "CrossEntropy", "exclude_missing": False}      # (a string, as in the reference)
    two_d = {"batch_size": 128, "transform_degree": 0, "filters": [64, 128, 256, 512, 1024], "use_res_units": False,
             "downsample": False, "lr": 0.001, "loss_fx": ["Focal", "Dice"], "exclude_missing": False}
    want = {BaseUNet3D: three_d, BaseUNet2D: two_d, MixupUNet2D: two_d}
    order = ["batch_size", "transform_degree", "filters", "use_res_units", "downsample", "lr", "loss_fx", "exclude_missing"]
    batch_help = {BaseUNet3D: "Volumes per optimizer step", BaseUNet2D: "Slices per optimizer step",
                  MixupUNet2D: "Slices per optimizer step"}
    for cls, defaults in want.items():
        parser = cls.add_model_specific_args(ArgumentParser(add_help=False))
        got = vars(parser.parse_args([]))
        assert got == defaults and list(got) == order, (cls.__name__, got)
        assert [a.dest for a in parser._actions] == order and parser._actions[0].help == batch_help[cls]
        assert parser.parse_args(["--loss_fx", "Dice", "Focal", "--filters", "4", "8", "16", "32", "64"]).loss_fx == ["Dice", "Focal"]
