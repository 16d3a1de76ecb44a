"""One dq_row_outcomes call over synthetic validity bitmaps, for a kernel trace of row_outcomes_kernel:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_rowlevel.py --rows 100000000

4 NOT_NULL terms over 2 checks (2 each), no `where`: the kernel reads 4 x n/8 bytes and writes, per check, the n-byte
BOOLEAN column and the n/8-byte pass bitmap. Prints one JSON line with the counts and the algorithmic bytes."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import deequ_amd.native as N  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--null", action="store_true", help="filteredRow = null (adds one n/8-byte validity bitmap per check)")
    args = ap.parse_args()
    import torch
    n = args.rows
    ctx = N.context(0)
    dev = torch.device("cuda", 0)
    nwords = (n + 63) // 64
    values = torch.zeros(n, dtype=torch.uint8, device=dev)
    cols, keep = [], [values]
    for c in range(4):
        validity = torch.zeros(nwords * 8, dtype=torch.uint8, device=dev)
        ctx.synth_validity(1234 + c, 0, n, 100 * (c + 1), validity.data_ptr())
        col = N.DqColumn()
        col.spark_type, col.flags, col.length = N.TYPE_BOOLEAN, N.COL_DEVICE, n
        col.values, col.validity = values.data_ptr(), validity.data_ptr()
        cols.append(col)
        keep.append(validity)
    terms = []
    for c in range(4):
        t = N.DqRowTerm()
        t.kind, t.index, t.where, t.check = N.ROW_NOT_NULL, c, -1, c // 2
        terms.append(t)
    checks = []
    for _ in range(2):
        ck = N.DqRowCheck()
        bufs = [torch.empty(nwords * 8, dtype=torch.uint8, device=dev),
                torch.empty((n + 15) // 16 * 16, dtype=torch.uint8, device=dev),
                torch.empty(nwords * 8, dtype=torch.uint8, device=dev)]
        ck.pass_bits, ck.values, ck.validity = (b.data_ptr() for b in bufs)
        checks.append(ck)
        keep.extend(bufs)
    flags = N.ROW_FILTERED_NULL if args.null else 0
    for _ in range(args.calls):
        tc, cc = ctx.row_outcomes(cols, n, [], terms, checks, flags)
    read = 4 * (n // 8)
    written = 2 * (n + n // 8 + (n // 8 if args.null else 0))
    print(json.dumps({"rows": n, "terms": 4, "checks": 2, "filteredRow": "null" if args.null else "true", "term_counts": tc,
                      "check_counts": cc, "bytes_read": read, "bytes_written": written}))


if __name__ == "__main__":
    main()
