#!/usr/bin/env python
"""One-GPU timing of the device CSV reader (not bench.py). Generates a CSV of 8 columns (int, long, double, boolean,
short strings, quoted strings with commas, a second int and double; 5 % empty fields) at --rows rows (default 1e6 and
1e7), then times, each best of --reps after a warm-up and reported separately:
  upload      the file's bytes host -> HBM (one torch copy)
  parse       dq_csv_index + one dq_csv_column per column over the resident bytes (Table.from_csv(device=) minus the
              file read and the upload), with bytes/s against the 6.29 TB/s copy ceiling of DESIGN.md §3
  from_csv    Table.from_csv(path, device=0) whole: file read + upload + parse
  host        Table.from_csv(path) + to_device, at --host-rows rows at the most (per-cell Python: too slow beyond)
  pyarrow     pyarrow.csv.read_csv + Table.from_arrow + to_device (Arrow's typing, not Spark's)
Prints the lines and writes them to --out."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING = 6.29e12  # B/s, DESIGN.md §3


def best_ms(fn, warmup, reps):
    best = None
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        ms = (time.perf_counter() - t0) * 1e3
        if k >= warmup:
            best = ms if best is None else min(best, ms)
    return best


def generate(path, rows, seed=1):
    """The benchmark file, written in blocks with numpy (no per-cell Python)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    words = np.array(["alpha", "beta", "gamma", "delta", "epsilon", "zeta", "eta", "theta"])
    with open(path, "w", newline="") as f:
        f.write("id,big,price,flag,word,note,qty,ratio\n")
        done = 0
        while done < rows:
            n = min(200_000, rows - done)
            cols = [
                (np.arange(done, done + n)).astype(str),
                rng.integers(-2 ** 62, 2 ** 62, n).astype(str),
                np.round(rng.normal(100.0, 30.0, n), 6).astype(str),
                np.where(rng.random(n) < 0.5, "true", "false"),
                words[rng.integers(0, len(words), n)],
                np.char.add(np.char.add('"', np.char.add(words[rng.integers(0, len(words), n)], ", ")),
                            np.char.add(words[rng.integers(0, len(words), n)], '"')),
                rng.integers(-1000, 1000, n).astype(str),
                rng.random(n).astype(str),
            ]
            for c in range(1, len(cols)):  # 5 % empty fields (not the id)
                cols[c] = np.where(rng.random(n) < 0.05, "", cols[c])
            block = cols[0]
            for c in cols[1:]:
                block = np.char.add(np.char.add(block, ","), c)
            f.write("\n".join(block.tolist()) + "\n")
            done += n
    return os.path.getsize(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--host-rows", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device-only", action="store_true", help="skip the host and pyarrow readers (profiling runs)")
    ap.add_argument("--dir", default=None, help="where the generated files go (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "bench_csv.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from deequ_amd import engine
    from deequ_amd import table as T
    from deequ_amd.table import Table
    ctx = engine.ctx()
    dev = torch.device("cuda", engine.device())
    lines = []

    def line(txt):
        print(txt, flush=True)
        lines.append(txt)

    tmp = tempfile.TemporaryDirectory() if args.dir is None else None
    where = args.dir or tmp.name
    for rows in args.rows:
        path = os.path.join(where, "bench_%d.csv" % rows)
        t0 = time.perf_counter()
        nbytes = generate(path, rows)
        line("file: %d rows x 8 columns, %d bytes (%.1f B/row), generated in %.1f s"
             % (rows, nbytes, nbytes / rows, time.perf_counter() - t0))
        raw = np.fromfile(path, dtype=np.uint8)
        held = {}

        def upload():
            held["data"] = torch.from_numpy(raw).to(dev)
            torch.cuda.synchronize(dev)

        ms = best_ms(upload, args.warmup, args.reps)
        line("upload: %.2f ms, %.1f GB/s" % (ms, nbytes / ms / 1e6))
        data = held["data"]
        names = T._csv_first_record(raw[:1 << 16].tobytes())[0]

        def parse():
            handle, res, reports = ctx.csv_index(data.data_ptr(), nbytes, len(names), 1)
            assert not res.refusal_kind and res.nrows == rows
            out = []
            try:
                for j, rep in enumerate(reports):
                    t = T._csv_type_of_classes(rep.classes)
                    val = torch.zeros((rows + 63) // 64 * 8, dtype=torch.uint8, device=dev) if rep.valid < rows else None
                    vp = val.data_ptr() if val is not None else None
                    if t == T.N.TYPE_STRING:
                        off = torch.empty(rows + 1, dtype=torch.int32, device=dev)
                        total = ctx.csv_column(handle, j, t, None, vp, off.data_ptr())
                        vals = torch.empty(total + 16, dtype=torch.uint8, device=dev)
                        ctx.csv_column(handle, j, t, vals.data_ptr(), None, off.data_ptr())
                        out.append((vals, off, val))
                    else:
                        vals = torch.empty(rows * np.dtype(T.NUMPY_OF[t]).itemsize, dtype=torch.uint8, device=dev)
                        ctx.csv_column(handle, j, t, vals.data_ptr(), vp)
                        out.append((vals, val))
            finally:
                ctx.csv_free(handle)
            held["cols"] = out

        ms = best_ms(parse, args.warmup, args.reps)
        line("parse (index + 8 columns, bytes resident): %.2f ms, %.2f Mrows/s, %.2f GB/s of file bytes = %.2f %% of the "
             "%.2f TB/s copy ceiling" % (ms, rows / ms / 1e3, nbytes / ms / 1e6, 100 * nbytes / (ms / 1e3) / COPY_CEILING,
                                        COPY_CEILING / 1e12))
        held.clear()
        del data

        def whole():
            held["t"] = Table.from_csv(path, device=dev.index)

        ms = best_ms(whole, args.warmup, args.reps)
        line("from_csv(device): %.2f ms, %.2f Mrows/s; schema %s" % (ms, rows / ms / 1e3, dict(held["t"].schema)))
        held.clear()

        if args.device_only:
            os.remove(path)
            continue
        if rows <= args.host_rows:
            def host():
                held["t"] = Table.from_csv(path).to_device(dev.index)
                torch.cuda.synchronize(dev)

            ms = best_ms(host, 0, 1)
            line("host from_csv + to_device (%d rows, one run): %.0f ms, %.3f Mrows/s" % (rows, ms, rows / ms / 1e3))
            held.clear()
        else:
            line("host from_csv + to_device: not taken at %d rows (per-cell Python; taken up to %d rows)"
                 % (rows, args.host_rows))

        import pyarrow.csv as pacsv

        def arrow():
            held["t"] = Table.from_arrow(pacsv.read_csv(path)).to_device(dev.index)
            torch.cuda.synchronize(dev)

        ms = best_ms(arrow, args.warmup, args.reps)
        line("pyarrow.csv.read_csv + from_arrow + to_device: %.2f ms, %.2f Mrows/s (Arrow's typing: %s)"
             % (ms, rows / ms / 1e3, dict(held["t"].schema)))
        held.clear()
        os.remove(path)
    line("csv kernel launches: %r" % ctx.csv_kernel_launches())
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
