"""Time Table.from_arrow(t, device=0) against from_arrow(t).to_device(0) on one seeded Arrow table.

    python tools/bench_ingest.py --rows 1e7 --rows 1e8

The table is built from a seed, no files: two int64, two float64, one int32, one boolean, one ns timestamp and one short
string column, 5 % NULLs, Arrow chunks of 2^20 rows. After one warm-up of each path the two are timed alternately,
`--repeats` times each, with a host clock around a device synchronise; the medians are compared. One JSON line per size.
`--device-only` runs the new path alone (for a kernel trace in a run of its own)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK = 1 << 20


def build_table(rows, seed):
    import pyarrow as pa
    cols = {n: [] for n in ("a", "b", "x", "y", "k", "flag", "ts", "s")}
    for c, r0 in enumerate(range(0, rows, CHUNK)):
        m = min(CHUNK, rows - r0)
        rng = np.random.default_rng([seed, c])

        def nulls():
            return rng.random(m) < 0.05

        cols["a"].append(pa.array(rng.integers(-2 ** 62, 2 ** 62, m), mask=nulls()))
        cols["b"].append(pa.array(rng.integers(0, 1000, m), mask=nulls()))
        cols["x"].append(pa.array(rng.normal(10.0, 3.0, m), mask=nulls()))
        cols["y"].append(pa.array(rng.random(m), mask=nulls()))
        cols["k"].append(pa.array(rng.integers(-2 ** 31, 2 ** 31, m).astype(np.int32), mask=nulls()))
        cols["flag"].append(pa.array(rng.random(m) < 0.5, mask=nulls()))
        cols["ts"].append(pa.array(rng.integers(0, 2 * 10 ** 18, m), type=pa.int64(), mask=nulls())
                          .cast(pa.timestamp("ns")))
        lens = rng.integers(0, 9, m)
        offs = np.zeros(m + 1, dtype=np.int32)
        np.cumsum(lens, out=offs[1:])
        data = rng.integers(97, 123, int(offs[-1]), dtype=np.uint8)
        valid = np.packbits(~nulls(), bitorder="little")
        cols["s"].append(pa.Array.from_buffers(pa.string(), m, [pa.py_buffer(valid.tobytes()), pa.py_buffer(offs.tobytes()),
                                                                pa.py_buffer(data.tobytes())], null_count=-1))
    return pa.table({n: pa.chunked_array(v) for n, v in cols.items()})


def device_bytes(table):
    total = 0
    for col in table.columns.values():
        total += sum(t.numel() * t.element_size() for t in col.device.values())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, action="append")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    import torch
    from deequ_amd.table import Table
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest.py needs the GPU: nothing is measured without it")
    dev = torch.device("cuda", 0)

    def timed(f):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    # the yardstick of an upload: one pageable host buffer copied whole, as §3i measured it for a file's bytes
    block = np.ones(1 << 30, dtype=np.uint8)
    timed(lambda: torch.from_numpy(block).to(dev))
    copy_s = statistics.median(timed(lambda: torch.from_numpy(block).to(dev))[0] for _ in range(3))
    del block
    for rows in [int(r) for r in (args.rows or [1e7])]:
        t0 = time.perf_counter()
        table = build_table(rows, args.seed)
        build_s = time.perf_counter() - t0
        new = lambda: Table.from_arrow(table, device=0)  # noqa: E731
        old = lambda: Table.from_arrow(table).to_device(0)  # noqa: E731
        nbytes = device_bytes(timed(new)[1])  # warm-up
        old_s, new_s = [], []
        if not args.device_only:
            timed(old)
        for _ in range(args.repeats):
            if not args.device_only:
                old_s.append(timed(old)[0])
            new_s.append(timed(new)[0])
        new_med = statistics.median(new_s)
        line = {"rows": rows, "arrow_chunks": table.column(0).num_chunks, "arrow_bytes": table.nbytes,
                "device_bytes": nbytes, "build_table_s": round(build_s, 3), "device_path_s": [round(x, 4) for x in new_s],
                "device_path_median_s": round(new_med, 4), "device_path_GBps": round(nbytes / new_med / 1e9, 2),
                "pageable_copy_1GiB_GBps": round((1 << 30) / copy_s / 1e9, 2)}
        if old_s:
            old_med = statistics.median(old_s)
            line.update({"host_path_s": [round(x, 4) for x in old_s], "host_path_median_s": round(old_med, 4),
                         "speedup": round(old_med / new_med, 2), "device_path_is_faster": new_med < old_med})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
