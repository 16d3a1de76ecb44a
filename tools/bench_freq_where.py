#!/usr/bin/env python
"""One-GPU timing of a filtered grouping (not bench.py): config C4's shape beside a filter column -- --rows LONG keys
with rows / 10 distinct values (dq_synth_freq_keys) and a LONG filter column, U[-2^31, 2^31), resident in HBM; the
filter `f < 0` keeps about half of the rows. Four times, each a whole call timed with HIP events on the context's
stream, best of --reps after --warmup, the two builds alternated rep by rep:
  1. dq_filter_validity: the predicate pass plus the mask launch (one target, the key column);
  2. the frequency-table build over the masked key column (dq_frequencies + dq_freq_summarize);
  3. the unfiltered build over the same column, with its run-to-run spread (max - min over the reps);
  4. Size(where) with the same predicate through dq_scan (the existing path that evaluates it), and, for reference,
     4b. the same call on the bitmap pass (DQ_WHERE_MASKS=0): the very predicate launch (1) runs, plus the bits scan.
Two bars, both against this binary's existing paths in this call: (2) no slower than (3) beyond the spread -- it reads
the same rows and inserts fewer keys -- and (1) no slower than (4) beyond the spread plus the mask kernel's own
traffic, (ntargets + 1) * rows / 8 bytes read and ntargets * rows / 8 written, at the copy rate of DESIGN.md §3.
Prints the lines and a verdict per bar; writes them to --out."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29  # the measured float4-copy ceiling


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500_000_000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "bench_freq_where.txt"))
    args = ap.parse_args()

    import torch
    import deequ_amd as D
    import deequ_amd.native as N
    from deequ_amd import engine
    from deequ_amd.table import Column, Table
    ctx = engine.ctx()
    dev = torch.device("cuda", engine.device())
    rows = args.rows
    distinct = max(2, rows // 10 // 2 * 2)
    if (rows - distinct) % (distinct // 2):
        raise SystemExit("--rows: (rows - rows / 10) must be a multiple of rows / 20 (dq_synth_freq_keys)")
    lines = []

    def line(txt):
        print(txt, flush=True)
        lines.append(txt)

    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    keys = torch.empty(rows, dtype=torch.int64, device=dev)
    filt = torch.empty(rows, dtype=torch.int64, device=dev)
    ctx.synth_freq_keys(rows, distinct, 0, rows, keys.data_ptr())
    ctx.synth_column(N.SYNTH_INT32R, 7, 0, rows, filt.data_ptr())
    ctx.synchronize()
    k = Column("k", N.TYPE_LONG, None, None, length=rows)
    k.device = {"values": keys}
    f = Column("f", N.TYPE_LONG, None, None, length=rows)
    f.device = {"values": filt}
    table = Table([k, f])
    where = "f < 0"
    batch = D.ScanBatch(table)
    pred = batch.preds[batch.predicate(where)]
    native = batch.native_columns()
    mask = torch.empty((rows + 63) // 64 * 8, dtype=torch.uint8, device=dev)
    size_op = N.DqOp()
    size_op.kind, size_op.where, size_op.predicate = N.OP_SIZE, 0, -1
    size_op.column[0], size_op.column[1] = -1, -1
    kept = {}

    def run_filter():
        kept["rows"] = ctx.filter_validity(native, rows, pred.to_native(), [0], [mask.data_ptr()])

    def run_size():
        kept["size"] = int(ctx.scan(native, rows, [size_op], [pred.to_native()])[0].u.num_matches.num_matches)

    def run_size_bitmaps():
        os.environ["DQ_WHERE_MASKS"] = "0"  # read per call
        try:
            run_size()
        finally:
            del os.environ["DQ_WHERE_MASKS"]

    def build(t):
        def run():
            ft = engine.frequencies(t, ["k"])
            kept["summary"] = ft.summary(None)
            del ft
        return run

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            fn()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed(fns):
        """{name: [ms per rep]} with the versions alternated rep by rep."""
        out = {name: [] for name, _ in fns}
        for r in range(args.warmup + args.reps):
            for name, fn in fns:
                ms = once(fn)
                if r >= args.warmup:
                    out[name].append(ms)
        return out

    torch.cuda.synchronize(dev)
    t1 = timed([("filter", run_filter), ("size", run_size), ("size_bitmaps", run_size_bitmaps)])
    assert kept["rows"] == kept["size"], kept
    masked = Column("k", N.TYPE_LONG, None, None, length=rows)
    masked.device = {"values": keys, "validity": mask}
    t2 = timed([("masked", build(Table([masked]))), ("plain", build(Table([k])))])
    assert kept["summary"]["num_rows"] == rows  # the last build is the unfiltered one
    once(build(Table([masked])))
    assert kept["summary"]["num_rows"] == kept["rows"], kept

    best = {name: min(v) for t in (t1, t2) for name, v in t.items()}
    spread = {name: max(v) - min(v) for t in (t1, t2) for name, v in t.items()}
    mask_ms = (2 * rows / 8 + rows / 8) / (COPY_TBS * 1e12) * 1e3
    line("rows %d, distinct %d, `%s` keeps %d rows (%.1f %%)" % (rows, distinct, where, kept["rows"],
                                                                 100.0 * kept["rows"] / rows))
    line("1 dq_filter_validity (predicate + mask launch): %.3f ms best of %d (spread %.3f ms)"
         % (best["filter"], args.reps, spread["filter"]))
    line("2 build over the masked column: %.3f ms best of %d (spread %.3f ms)" % (best["masked"], args.reps, spread["masked"]))
    line("3 unfiltered build: %.3f ms best of %d (spread %.3f ms; reps %s)"
         % (best["plain"], args.reps, spread["plain"], ", ".join("%.3f" % v for v in t2["plain"])))
    line("4 Size(where): %.3f ms best of %d (spread %.3f ms)" % (best["size"], args.reps, spread["size"]))
    line("4b Size(where) on the bitmap pass (DQ_WHERE_MASKS=0): %.3f ms best of %d (spread %.3f ms)"
         % (best["size_bitmaps"], args.reps, spread["size_bitmaps"]))
    line("mask kernel model: %.0f B read + %.0f B written at %.2f TB/s = %.3f ms" % (2 * rows / 8, rows / 8, COPY_TBS, mask_ms))
    ok2 = best["masked"] <= best["plain"] + spread["plain"]
    ok1 = best["filter"] <= best["size"] + spread["size"] + mask_ms
    line("bar A, (2) <= (3) + spread: %s (%.3f <= %.3f)" % ("met" if ok2 else "MISSED", best["masked"],
                                                          best["plain"] + spread["plain"]))
    line("bar B, (1) <= (4) + spread + mask model: %s (%.3f <= %.3f)" % ("met" if ok1 else "MISSED", best["filter"],
                                                                        best["size"] + spread["size"] + mask_ms))
    ctx.set_stream(None)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
