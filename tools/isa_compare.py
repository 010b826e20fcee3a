#!/usr/bin/env python3
"""Compare the gfx950 kernels of two built libctseg_hip.so files: what a refactor that is meant to change nothing is judged by.

Per kernel symbol, from the code objects inside each library (tools/isa_store_hazard.py: code_objects):
  * VGPR, AGPR, SGPR, LDS bytes and scratch bytes per lane from the code-object metadata (kernel_resources);
  * the disassembly with addresses, branch targets and symbol offsets stripped: `identical`, `same multiset` (the same
    instructions in another order) or `differs` with the instruction-count delta and the mnemonics that account for it.

    python tools/isa_compare.py OLD.so NEW.so [-v] [--only SUBSTRING]

Prints one line per kernel that is not identical (-v: every kernel) and a summary per source kernel name.  Exit code 1 if any
kernel changed VGPR, AGPR, LDS or scratch, or exists on one side only; an SGPR change is printed, not failed.
"""
import argparse
import collections
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_store_hazard as H  # noqa: E402

RES = ("vgpr", "agpr", "lds", "scratch")      # a change in one of these fails the comparison; SGPRs are reported only


def _normalise(mn, ops):
    """one instruction as a string, without what moves when code around it moves: branch targets and symbol offsets"""
    if mn.startswith("s_cbranch") or mn in ("s_branch", "s_call_b64"):
        return mn
    txt = mn + " " + ", ".join(ops)
    return re.sub(r"<[^>]*>", "", re.sub(r"\b0x[0-9a-f]+\b(?=\s*<)", "", txt)).strip()


def kernels(lib_path):
    """{kernel symbol: {"res": {...}, "ins": [normalised instruction]}} of every gfx950 kernel in the library"""
    ins = collections.defaultdict(list)
    for _, obj in H.code_objects(lib_path):
        for sym, mn, ops in H._instructions(H.disassemble(obj)):
            ins[sym].append(_normalise(mn, ops))
    return {sym: {"res": r, "ins": ins.get(sym, [])} for sym, r in H.kernel_resources(lib_path).items()}


def compare(old, new):
    """-> [(symbol, verdict, detail, resource changes)] over the union of both kernel sets; verdict in
    identical / multiset / differs / missing"""
    rows = []
    for sym in sorted(set(old) | set(new)):
        if sym not in old or sym not in new:
            rows.append((sym, "missing", "only in " + ("NEW" if sym in new else "OLD"), ["presence"]))
            continue
        a, b = old[sym], new[sym]
        changed = [f"{k} {a['res'][k]} -> {b['res'][k]}" for k in RES if a["res"][k] != b["res"][k]]
        note = "" if a["res"]["sgpr"] == b["res"]["sgpr"] else f"sgpr {a['res']['sgpr']} -> {b['res']['sgpr']}"
        if a["ins"] == b["ins"]:
            rows.append((sym, "identical", note, changed))
            continue
        ca, cb = collections.Counter(i.split()[0] for i in a["ins"]), collections.Counter(i.split()[0] for i in b["ins"])
        if collections.Counter(a["ins"]) == collections.Counter(b["ins"]):
            rows.append((sym, "multiset", note, changed))
            continue
        delta = {m: cb[m] - ca[m] for m in set(ca) | set(cb) if cb[m] != ca[m]}
        top = ", ".join(f"{m} {d:+d}" for m, d in sorted(delta.items(), key=lambda kv: (-abs(kv[1]), kv[0]))[:8])
        rows.append((sym, "differs", f"{len(b['ins']) - len(a['ins']):+d} instructions of {len(a['ins'])}" + (f" ({top})" if top else " (operands only)") + (f"; {note}" if note else ""), changed))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("-v", "--verbose", action="store_true", help="list identical kernels too, with their resource numbers")
    ap.add_argument("--only", default="", help="only kernels whose demangled name contains this")
    args = ap.parse_args(argv)
    old, new = kernels(args.old), kernels(args.new)
    rows = compare(old, new)
    dem = dict(zip([r[0] for r in rows], subprocess.check_output(["c++filt"], input="\n".join(r[0] for r in rows), text=True).splitlines()))
    rows = [r for r in rows if args.only in dem[r[0]]]
    family = collections.defaultdict(collections.Counter)
    bad = 0
    for sym, verdict, detail, changed in rows:
        family[re.sub(r"^void ", "", dem[sym]).split("<")[0].split("(")[0]][verdict] += 1
        bad += bool(changed)
        if args.verbose or verdict != "identical" or changed:
            r = (new.get(sym) or old[sym])["res"]
            print(f"{verdict:9s} {dem[sym][:150]}\n          " + " ".join(f"{k}={r[k]}" for k in RES + ("sgpr",)) + (f"  {detail}" if detail else "") +
                  (f"  RESOURCES CHANGED: {'; '.join(changed)}" if changed else ""))
    print(f"\n{len(rows)} kernels")
    for name, c in sorted(family.items()):
        if args.verbose or set(c) != {"identical"}:
            print(f"  {name}: " + ", ".join(f"{c[v]} {v}" for v in ("identical", "multiset", "differs", "missing") if c[v]))
    print(f"{sum(c['identical'] for c in family.values())} identical, {sum(c['multiset'] for c in family.values())} same multiset, "
          f"{sum(c['differs'] for c in family.values())} differ, {bad} with changed resources")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
