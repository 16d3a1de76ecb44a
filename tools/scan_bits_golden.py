"""Record the striped scan's state bits: tests/golden/striped_scan_bits.json (needs the GPU).

    python tools/scan_bits_golden.py [--force]

Runs Size plus the six C2 analyzers per column over the inputs of tests/striped_bits_cases.py at DQ_SCAN_GRID = 1, 2
and 3 with the library that is loaded (DQ_LIBRARY selects another build) and writes every field of every state as
hex. Run it from the commit whose results are the reference, before a change to the kernel's instruction stream;
tests/test_gpu_scan_striped_bits.py then holds the changed kernel to those bits. An existing file is only replaced
with --force.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true", help="replace an existing golden file")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import striped_bits_cases as C
    out = a.out or C.GOLDEN
    if os.path.exists(out) and not a.force:
        sys.exit("%s exists; pass --force to replace it" % out)
    golden = {"cases": {}}
    for key, build in C.cases():
        table = build().to_device()
        analyzers = C.analyzers_of(table)
        for grid in ((2,) if key.startswith("late/") else C.GRIDS):
            os.environ["DQ_SCAN_GRID"] = str(grid)
            golden["cases"]["%s/grid=%d" % (key, grid)] = {
                repr(an): C.encode(st) for an, st in zip(analyzers, C.run_states(table, analyzers))}
    os.environ.pop("DQ_SCAN_GRID", None)
    with open(out, "w") as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases" % (out, len(golden["cases"])))


if __name__ == "__main__":
    main()
