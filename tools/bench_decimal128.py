#!/usr/bin/env python
"""One-GPU timing of the decimal128 scan (not bench.py): one DECIMAL128 column of --rows rows with 5 % NULLs, resident
in HBM, through dq_scan. Two configurations: Sum + Minimum + Maximum + Completeness (count / sum / compare only: the
memory-bound shape, 16.125 B per row), and the same plus StandardDeviation and ApproxCountDistinct, once over a column
whose cells all take dec128_to_double's fast path (|unscaled| < 2^53, scale 18) and once over one whose cells all take
the long division (|unscaled| up to 2^100). Each dq_scan call is timed with HIP events on the context's stream (plan
upload, the decimal128 launch, the fold and the state download), best of --reps after --warmup. Prints ms, rows/s and
bytes/s beside the int64 launch's 6.25 TB/s (profiles/r06/c2_kernel_stats_r06m.csv); writes the lines to --out."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INT64_YARDSTICK_TBS = 6.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=250_000_000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "bench_decimal128.txt"))
    args = ap.parse_args()

    import torch
    import deequ_amd.native as N
    from deequ_amd import engine
    from deequ_amd.table import Column
    ctx = engine.ctx()
    dev = torch.device("cuda", engine.device())
    rows = args.rows
    lines = []

    def line(txt):
        print(txt, flush=True)
        lines.append(txt)

    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    validity = torch.zeros((rows + 63) // 64 * 8, dtype=torch.uint8, device=dev)
    ctx.synth_validity(11, 0, rows, 50, validity.data_ptr())
    ctx.synchronize()

    def column(lo, hi):
        cells = torch.stack([lo, hi], dim=1).contiguous()  # (rows, 2) int64 = little-endian (lo, hi) limbs
        col = Column("x", N.TYPE_DECIMAL128, None, None, decimal_precision=38, decimal_scale=18, length=rows)
        col.device = {"values": cells.view(torch.uint8).reshape(-1), "validity": validity}
        return col

    def ops_of(kinds):
        out = []
        for k in kinds:
            op = N.DqOp()
            op.kind, op.where, op.predicate = k, -1, -1
            op.column[0], op.column[1] = 0, -1
            out.append(op)
        return out

    def timed(col, kinds):
        native, ops = [col.native()], ops_of(kinds)
        torch.cuda.synchronize(dev)  # the generators ran on torch's stream
        best = None
        for k in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record()
                states = ctx.scan(native, rows, ops, [])
                e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if k >= args.warmup:
                best = ms if best is None else min(best, ms)
        assert all(s.present for s in states)
        return best

    def report(name, col, kinds):
        ms = timed(col, kinds)
        nbytes = rows * 16 + rows / 8
        tbs = nbytes / ms / 1e9
        line("%s: %d rows, 5 %% NULLs: %.3f ms, %.1f Grows/s, %.2f TB/s (%.0f %% of the int64 launch's %.2f TB/s)"
             % (name, rows, ms, rows / ms / 1e6, tbs, 100.0 * tbs / INT64_YARDSTICK_TBS, INT64_YARDSTICK_TBS))

    light = [N.OP_SUM, N.OP_MINIMUM, N.OP_MAXIMUM, N.OP_COMPLETENESS]
    heavy = light + [N.OP_STANDARD_DEVIATION, N.OP_APPROX_COUNT_DISTINCT]
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    small = torch.randint(-(1 << 52), 1 << 52, (rows,), dtype=torch.int64, device=dev, generator=gen)
    fast = column(small, small >> 63)
    del small
    report("Sum+Min+Max+Completeness", fast, light)
    report("+StandardDeviation+ApproxCountDistinct, fast-path cells", fast, heavy)
    del fast
    lo = torch.randint(-(1 << 62), 1 << 62, (rows,), dtype=torch.int64, device=dev, generator=gen)
    hi = torch.randint(-(1 << 36), 1 << 36, (rows,), dtype=torch.int64, device=dev, generator=gen)
    hi = torch.where(hi == 0, torch.ones_like(hi), torch.where(hi == -1, torch.full_like(hi, -2), hi))
    slow = column(lo, hi)
    del lo, hi
    report("Sum+Min+Max+Completeness, long-division cells", slow, light)
    report("+StandardDeviation+ApproxCountDistinct, long-division cells", slow, heavy)
    ctx.set_stream(None)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
