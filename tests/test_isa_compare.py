"""CPU: tools/isa_compare.py, the kernel-by-kernel comparison of two built libraries that refactors are judged by, keeps working:
run on the built library against itself it finds every kernel, and no difference."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_compare as C  # noqa: E402
import isa_store_hazard as H  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(H.LLVM, "llvm-objdump")) or not os.path.exists(H.DEFAULT_LIB),
                                reason="ROCm LLVM tools missing or the library is not built")


def test_library_against_itself_has_no_differences(capsys):
    ks = C.kernels(H.DEFAULT_LIB)
    assert len(ks) > 200                                                   # every translation unit's kernels were found
    assert all(len(k["ins"]) > 0 for k in ks.values())                     # ... and disassembled under their own symbol
    some = next(k for s, k in ks.items() if "conv_halo_x_kernel" in s)
    assert {"vgpr", "agpr", "sgpr", "lds", "scratch"} <= set(some["res"]) and some["res"]["vgpr"] > 0 and some["res"]["lds"] > 0
    rows = C.compare(ks, ks)
    assert len(rows) == len(ks) and all(v == "identical" and not changed for _, v, _, changed in rows)
    assert C.main([H.DEFAULT_LIB, H.DEFAULT_LIB]) == 0
    assert f"{len(ks)} identical, 0 same multiset, 0 differ, 0 with changed resources" in capsys.readouterr().out


def test_a_changed_kernel_is_reported():
    a = {"k": {"res": {"vgpr": 10, "agpr": 0, "sgpr": 20, "lds": 0, "scratch": 0}, "ins": ["s_mov_b32 s0, s1", "v_add_f32 v0, v1, v2", "s_endpgm"]}}
    swapped = {"k": {"res": dict(a["k"]["res"]), "ins": ["v_add_f32 v0, v1, v2", "s_mov_b32 s0, s1", "s_endpgm"]}}
    longer = {"k": {"res": dict(a["k"]["res"], vgpr=12), "ins": a["k"]["ins"][:2] + ["s_nop 0", "s_endpgm"]}}
    assert C.compare(a, swapped)[0][1:] == ("multiset", "", [])
    sym, verdict, detail, changed = C.compare(a, longer)[0]
    assert verdict == "differs" and detail.startswith("+1 instructions of 3") and "s_nop +1" in detail and changed == ["vgpr 10 -> 12"]
    sg = {"k": {"res": dict(a["k"]["res"], sgpr=21), "ins": list(a["k"]["ins"])}}
    assert C.compare(a, sg)[0] == ("k", "identical", "sgpr 20 -> 21", [])                 # reported, not a failure
    assert C.compare(a, {})[0][1] == "missing"
