"""tools/dump_plan.py (the canonical text of recorded plans that recorder refactors are compared with) keeps working: it records on
the CPU, and recording the same plan twice gives the same text."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_is_reproducible(monkeypatch):
    spec = importlib.util.spec_from_file_location("dump_plan", os.path.join(ROOT, "tools", "dump_plan.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(tool.nat, "require_gpu", tool.nat.require_gpu)       # dump() stubs it: restored after the test
    first, n_fwd, n_bwd = tool.dump("small_bf16")
    second, _, _ = tool.dump("small_bf16")
    assert n_fwd > 0 and n_bwd > 0 and first.count("\n") > n_fwd + n_bwd
    assert "fwd ctseg_conv_igemm {" in first and "bwd ctseg_conv_wgrad {" in first and "\nready [(" in first and "\npacker idx=" in first
    assert first == second
