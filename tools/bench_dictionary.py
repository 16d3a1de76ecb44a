#!/usr/bin/env python
"""One-GPU timing of dictionary-encoded string columns kept encoded against the same rows decoded (not bench.py).

One column of --rows rows with 5 % NULLs; dictionaries of 100 and 10 000 entries ("v<00000>"); uniform and single-hot
index distributions. Per case, in one process, HIP events around whole calls (best of 3 after a warm-up), kept and
decoded:
  scan      Completeness + ApproxCountDistinct + DataType + MaxLength (one ScanBatch.run)
  grouping  Uniqueness + Entropy (one AnalysisRunner run, DQ_RUN_SERIAL)
  pattern   PatternMatch (one ScanBatch.run)
and the yardstick of dict_counts_kernel: the striped scan (Completeness + Sum) over the same int32 buffer as an INT
column. `--ingest` instead times Table.from_parquet of one file with and without dictionaries="keep" on the CPU;
`--copies` times dq_dict_counts alone per number of LDS counter copies and on the global-atomic path.
Prints one line per measurement; writes the same lines to --out."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(rows, nd, hot, seed=1):
    import numpy as np
    from deequ_amd.table import DictColumn, Table, _column_from_pylist, pack_validity
    rng = np.random.default_rng(seed)
    idx = np.full(rows, nd // 3, dtype=np.int32) if hot else rng.integers(0, nd, rows, dtype=np.int32)
    valid = rng.random(rows, dtype=np.float32) >= 0.05
    idx[~valid] = 0
    entries = _column_from_pylist("cat", "string", ["v%05d" % i for i in range(nd)])
    col = DictColumn("cat", idx, pack_validity(valid), entries)
    return Table([col]).to_device(0)


class Timer:
    def __init__(self, torch, stream):
        self.torch, self.stream = torch, stream

    def ms(self, fn, warmup=1, reps=3):
        best = None
        for k in range(warmup + reps):
            a, b = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
            a.record(self.stream)
            fn()
            b.record(self.stream)
            b.synchronize()
            if k >= warmup:
                t = a.elapsed_time(b)
                best = t if best is None else min(best, t)
        return best


def gpu(args, emit):
    import torch
    import deequ_amd as D
    import deequ_amd.native as N
    from deequ_amd import engine
    from deequ_amd.table import Column, Table
    os.environ["DQ_RUN_SERIAL"] = "1"
    ctx = engine.ctx()
    stream = torch.cuda.Stream(device=engine.device())
    ctx.set_stream(stream.cuda_stream)
    timer = Timer(torch, stream)
    rows = int(float(args.rows))

    def scan(table, analyzers):
        def run():
            batch = D.ScanBatch(table)
            for a in analyzers:
                a.addOps(batch)
            batch.run()
        return run

    def grouping(table):
        return lambda: D.AnalysisRunner.onData(table).addAnalyzers([D.Uniqueness(["cat"]), D.Entropy("cat")]).run()

    for nd in (100, 10_000):
        for hot in (False, True):
            kept = build(rows, nd, hot)
            dcol = kept["cat"]
            t0 = time.perf_counter()
            plain = dcol.decoded()
            decode_s = time.perf_counter() - t0
            decoded = Table([plain])
            ints = Column("cat", N.TYPE_INT, None, None, length=rows)
            ints.device = {"values": dcol.dict_device["indices"], "validity": dcol.dict_device["validity"]}
            ints = Table([ints])
            tag = "rows=%d entries=%d dist=%s" % (rows, nd, "hot" if hot else "uniform")
            emit("%s device_decode_ms=%.2f decoded_bytes=%d" % (tag, decode_s * 1e3, plain.device["values"].numel() - 16))
            stripe = timer.ms(scan(ints, [D.Completeness("cat"), D.Sum("cat")]))
            emit("%s yardstick striped_scan_int32_ms=%.3f GB/s=%.0f" % (tag, stripe, rows * 4.125 / stripe / 1e6))
            configs = (("scan", lambda t: scan(t, [D.Completeness("cat"), D.ApproxCountDistinct("cat"), D.DataType("cat"),
                                                   D.MaxLength("cat")])),
                       ("grouping", grouping),
                       ("pattern", lambda t: scan(t, [D.PatternMatch("cat", r"^v\d+7$")])))
            for name, make in configs:
                k, d = timer.ms(make(kept)), timer.ms(make(decoded))
                emit("%s config=%s kept_ms=%.3f decoded_ms=%.3f ratio=%.2f kept_GB/s=%.0f"
                     % (tag, name, k, d, d / k, rows * 4.125 / k / 1e6))
            del kept, decoded, ints, plain, dcol
            torch.cuda.empty_cache()


def copies(args, emit):
    """dq_dict_counts alone for 1, 2, 4 and 8 LDS counter copies (DQ_DICT_LDS_COPIES) and the global-atomic path
    (DQ_DICT_LDS_ENTRIES=0), over uniform, single-hot and mixed (80 % one value, the rest uniform) indices."""
    import numpy as np
    import torch
    from deequ_amd import engine
    ctx = engine.ctx()
    stream = torch.cuda.Stream(device=engine.device())
    ctx.set_stream(stream.cuda_stream)
    timer = Timer(torch, stream)
    rows = int(float(args.rows))
    for nd in (100, 1000):
        for dist in ("uniform", "hot", "mixed"):
            kept = build(rows, nd, dist == "hot")
            col = kept["cat"]
            if dist == "mixed":
                rng = np.random.default_rng(3)
                idx = col.indices.copy()
                idx[rng.random(rows, dtype=np.float32) < 0.8] = nd // 3
                col.indices = idx
                col.to_device(0)
            counts = torch.empty(nd, dtype=torch.int64, device=col.dict_device["indices"].device)
            native = col.native_dict()
            for setting in ("1", "2", "4", "8", "global"):
                os.environ.pop("DQ_DICT_LDS_COPIES", None)
                os.environ.pop("DQ_DICT_LDS_ENTRIES", None)
                if setting == "global":
                    os.environ["DQ_DICT_LDS_ENTRIES"] = "0"
                else:
                    os.environ["DQ_DICT_LDS_COPIES"] = setting
                ms = timer.ms(lambda: ctx.dict_counts(native, counts.data_ptr()))
                emit("counts rows=%d entries=%d dist=%s copies=%s dq_dict_counts_ms=%.3f GB/s=%.0f"
                     % (rows, nd, dist, setting, ms, rows * 4.125 / ms / 1e6))
            os.environ.pop("DQ_DICT_LDS_COPIES", None)
            os.environ.pop("DQ_DICT_LDS_ENTRIES", None)
            del kept, col, counts
            torch.cuda.empty_cache()


def ingest(args, emit):
    import numpy as np
    import pyarrow as pa
    import pyarrow.parquet as pq
    import tempfile
    from deequ_amd.table import Table
    rows = int(float(args.rows))
    rng = np.random.default_rng(2)
    for nd in (100, 10_000):
        entries = np.array(["v%05d" % i for i in range(nd)], dtype=object)
        arr = pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, nd, rows, dtype=np.int32), mask=rng.random(rows) < 0.05),
                                             pa.array(entries, type=pa.string()))
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "t.parquet")
            pq.write_table(pa.table({"cat": arr}), path)
            for mode in ("decode", "keep"):
                best = None
                for _ in range(3):
                    t0 = time.perf_counter()
                    Table.from_parquet(path, dictionaries=mode)
                    dt = time.perf_counter() - t0
                    best = dt if best is None else min(best, dt)
                emit("ingest rows=%d entries=%d dictionaries=%s from_parquet_ms=%.1f" % (rows, nd, mode, best * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="2.5e8")
    ap.add_argument("--ingest", action="store_true")
    ap.add_argument("--copies", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
    (ingest if args.ingest else copies if args.copies else gpu)(args, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
