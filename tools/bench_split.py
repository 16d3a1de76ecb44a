#!/usr/bin/env python
"""One-GPU timing of the train / test row split (not bench.py): dq_split_rows alone over --rows rows (both bitmaps,
counts; the call returns after its stream synchronised, so wall time is the time of the call), then the whole
split_train_test of one GPU's C5 shard (bench.py's c5_shard: 10 fixed-width and 10 string columns, two row chunks at
2.5e8 rows). Prints ms, rows/s and the bytes the split writes; writes the same lines to --out."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best_ms(fn, warmup, reps):
    best = None
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        ms = (time.perf_counter() - t0) * 1e3
        if k >= warmup:
            best = ms if best is None else min(best, ms)
    return best


def device_bytes(table):
    from deequ_amd.table import ChunkedTable
    chunks = table.chunks if isinstance(table, ChunkedTable) else [table]
    return sum(v.numel() * v.element_size() for t in chunks for c in t.columns.values() for v in c.device.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=250_000_000)
    ap.add_argument("--ratio", type=float, default=0.1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "bench_split.txt"))
    args = ap.parse_args()

    import torch
    import bench
    import deequ_amd as D
    import deequ_amd.native as N
    from deequ_amd import engine
    ctx = engine.ctx()
    dev = torch.device("cuda", engine.device())
    rows = args.rows
    lines = []

    def line(txt):
        print(txt, flush=True)
        lines.append(txt)

    nb = (rows + 63) // 64 * 8
    train, test = (torch.zeros(nb, dtype=torch.uint8, device=dev) for _ in range(2))
    counts = {}

    def split():
        counts["c"] = ctx.split_rows(rows, 0, 0, args.ratio, train.data_ptr(), test.data_ptr())

    ms = best_ms(split, args.warmup, args.reps)
    line("dq_split_rows: %d rows, ratio %g: %.3f ms, %.1f Grows/s, %.1f GB/s written (train %d, test %d)"
         % (rows, args.ratio, ms, rows / ms / 1e6, 2 * nb / ms / 1e6, counts["c"][0], counts["c"][1]))
    del train, test

    t, nbytes = bench.c5_shard(torch, N, ctx, dev, rows)
    out = {}

    def whole():
        out.clear()  # release the previous outputs first
        out["r"] = D.split_train_test(t, args.ratio, 0)

    ms = best_ms(whole, args.warmup, args.reps)
    tr, te, _ = out["r"]
    line("split_train_test: C5 shard of %d rows x 20 columns (%.1f GB): %.1f ms, %.2f Grows/s; train %d + test %d rows, "
         "%.1f GB written" % (rows, nbytes / 1e9, ms, rows / ms / 1e6, tr.nrows, te.nrows,
                              (device_bytes(tr) + device_bytes(te)) / 1e9))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
