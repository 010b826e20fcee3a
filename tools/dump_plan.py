"""Record plans on the CPU (recording runs no kernel) and print them as canonical text, so that two versions of the recorder can be
compared byte for byte.

python tools/dump_plan.py [--list] [--out DIR] [CASE ...]      one line per case: name, SHA-1 of its text, ops in fwd / bwd

The text of a plan holds every op of ``fwd`` and ``bwd`` in order (name, scalar arguments, every field of a descriptor), the
gradient-readiness marks, the packer's index / description arrays as SHA-1 and the job tables of the batched slab reduces.
Pointers are written ``p<k>``, k = order of first appearance (``null`` for 0): allocation addresses drop out, aliasing, slicing,
buffer reuse and the order in which buffers are first mentioned stay visible.  A case whose recording raises is written as
the exception's type and message."""
import argparse
import ctypes as C
import gc
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-image-segmentation_amd")]
import torch  # noqa: E402
from capstone_amd import _native as nat  # noqa: E402
from capstone_amd.models import UNet  # noqa: E402

B = (3, 1, 10, (32, 64, 128, 256), (2, 2, 2, 2), 2)              # config B of bench.py: (dims, cin, cout, channels, strides, res units)
FULL = (2, 1, 512, 512, 48)
EMULATED = [                                                     # the CASES of tests/test_host_logic_emulated.py
    ((3, 1, 10, (4, 8, 16, 32), (2, 2, 2, 2), 2), (2, 1, 16, 16, 8)),
    ((3, 1, 10, (4, 8), (2,), 2), (1, 1, 8, 4, 6)),
    ((3, 2, 3, (4, 8, 12), (2, 2), 0), (1, 2, 8, 8, 4)),
    ((3, 1, 10, (8, 4, 8), (2, 2), 1), (1, 1, 8, 8, 8)),
    ((2, 1, 10, (4, 8, 16), (2, 2), 2), (2, 1, 16, 12)),
    ((2, 3, 5, (4, 8, 16), (2, 2), 0), (1, 3, 8, 8)),
]


def _case(net, shape, precision="bf16", norm="INSTANCE", train=True, inference=False, dx=False, env=None):
    return dict(net=net, shape=shape, precision=precision, norm=norm, train=train, inference=inference, dx=dx, env=env or {})


CASES = {
    "small_bf16": _case(B, (2, 1, 32, 32, 16)),
    "B_bf16": _case(B, FULL),
    "B_fp32": _case(B, FULL, "fp32"),
    "B_fp16_infer": _case(B, FULL, "fp16", inference=True),
    "B_bf16_bn_train": _case(B, FULL, norm="BATCH"),
    "B_bf16_bn_eval": _case(B, FULL, norm="BATCH", train=False, inference=True),
    "dx_2d_bf16": _case((2, 3, 5, (8, 16, 32), (2, 2), 2), (2, 3, 64, 48), dx=True),
    "dx_2d_fp32": _case((2, 3, 5, (4, 8, 16), (2, 2), 0), (1, 3, 8, 8), "fp32", dx=True),
    # 16-bit storage refuses the emulated cases' channel counts (not multiples of 8): their structures again with counts it takes
    "nores_bf16": _case((3, 2, 3, (8, 16, 24), (2, 2), 0), (1, 2, 16, 16, 8)),
    "equal_bottom_bf16": _case((3, 1, 10, (16, 8, 16), (2, 2), 1), (1, 1, 16, 16, 16)),
    "sliding_window_fp16": _case((3, 1, 10, (32, 64, 128, 256, 512), (2, 2, 2, 2), 2), (4, 1, 192, 192, 64), "fp16", inference=True),
}
for _i, (_net, _shape) in enumerate(EMULATED):
    for _p in ("fp32", "bf16"):
        CASES[f"emulated{_i}_{_p}"] = _case(_net, _shape, _p)
for _k, _v in (("CTSEG_BST", "0"), ("CTSEG_WGRAD_DYN", "0"), ("CTSEG_REDUCE_BATCH", "0"), ("CTSEG_NARROW_ROWS", "0"),
               ("CTSEG_NORM_ON_LOAD", "1"), ("CTSEG_WGRAD_TARGET_WGS", "512")):
    CASES[f"B_bf16_{_k}={_v}"] = _case(B, FULL, env={_k: _v})


def record(case):
    """the Plan of one case, recorded on the CPU"""
    dims, cin, cout, channels, strides, nres = case["net"]
    saved = {k: os.environ.get(k) for k in case["env"]}
    os.environ.update(case["env"])
    try:
        torch.manual_seed(0)
        net = UNet(dims, cin, cout, channels, strides, num_res_units=nres, precision=case["precision"], norm=case["norm"])
        net.train(case["train"])
        N, _, *sp = case["shape"]
        return net.engine().plan_for_shape("cpu", N, tuple(sp), inference=case["inference"], need_input_grad=case["dx"])
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def canon(plan):
    """canonical text of a recorded plan"""
    names = {}

    def ptr(v):
        return "p%d" % names.setdefault(v, len(names)) if v else "null"

    def value(v, is_ptr):
        if isinstance(v, C.Array):
            return "[" + ",".join(value(e, is_ptr) for e in v) + "]"
        if isinstance(v, C.Structure):
            return struct(v)
        return ptr(v) if is_ptr else repr(v)

    def struct(s):
        return "{" + " ".join(f"{nm}={value(getattr(s, nm), tp is C.c_void_p)}" for nm, tp, *_ in s._fields_) + "}"

    def sha(t):
        return "none" if t is None else hashlib.sha1(t.cpu().numpy().tobytes()).hexdigest()

    lines = []
    for tag, prog in (("fwd", plan.fwd), ("bwd", plan.bwd)):
        for name, fn, args in prog:
            assert len(args) + 1 == len(fn.argtypes), name                # (the stream is appended when the program runs)
            lines.append(f"{tag} {name} " + " ".join(value(v, tp is C.c_void_p) for v, tp in zip(args, fn.argtypes)))
            if name == "ctseg_conv_wgrad_reduce_batch":                   # its job table: a host tensor here, read in place
                for job in (nat.ReduceJob * args[1]).from_address(args[0]):
                    lines.append(f"{tag}   job {struct(job)}")
    lines.append("ready " + repr([(i, sorted(offs)) for i, offs in plan.ready_marks]))
    pk = plan.packer
    lines.append(f"packer idx={sha(pk.idx)} bias_idx={sha(pk.bias_idx)} pack_blocks={sha(pk.pack_blocks)} pack_rows={sha(pk.pack_rows)} "
                 f"n_first_rows={pk.n_first_rows} total={pk.total} bias_total={pk.bias_total}")
    return "\n".join(lines) + "\n"


def dump(name):
    """(text, ops in fwd, ops in bwd) of the named case"""
    nat.require_gpu = lambda t, what: None        # recording touches no device
    try:
        plan = record(CASES[name])
    except Exception as e:                        # part of the recorder's behaviour: compared like a program
        return f"raised {type(e).__name__}: {e}\n", 0, 0
    out = canon(plan), len(plan.fwd), len(plan.bwd)
    del plan
    gc.collect()            # a plan is a reference cycle holding gigabytes of buffers: free it before the next case is recorded
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("cases", nargs="*", help="default: all")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--out", help="directory that receives <case>.txt")
    a = ap.parse_args()
    if a.list:
        print("\n".join(CASES))
        return
    for name in a.cases or CASES:
        text, nf, nb = dump(name)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, name + ".txt"), "w") as f:
                f.write(text)
        print(name, hashlib.sha1(text.encode()).hexdigest(), nf, nb, flush=True)


if __name__ == "__main__":
    main()
