#!/usr/bin/env python
"""One-GPU timing of the device CSV writer (not bench.py). The table is tools/bench_csv.py's file (8 columns: int,
long, double, boolean, short strings, strings with commas, a second int and double; 5 % NULL cells) read by
Table.from_csv(path, device=0), at --rows rows (default 1e6 and 1e7). Each figure is the best of --reps after a
warm-up, reported separately:
  size        dq_csv_write_size: the mark pass of the two string columns, the row sizes, the scan
  write       dq_csv_write: the mark pass again, then the body into a device buffer
  download    the body HBM -> host (one torch copy)
  file        the host bytes into a file
  to_csv      Table.to_csv(path) whole
with bytes/s of size + write against the 6.29 TB/s copy ceiling of DESIGN.md §3. Yardsticks of the same run, none of
them the code under test:
  pyarrow     Table.to_arrow() (the download) and pyarrow.csv.write_csv of that table: the multi-threaded CPU writer;
              its number formatting is Arrow's, not Java's, so its file differs
  parse       the device reader over the written file (dq_csv_index + one dq_csv_column per column, bytes resident)
--device-only runs the size and write calls alone (profiling runs). Prints the lines and writes them to --out."""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_csv import COPY_CEILING, best_ms, generate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device-only", action="store_true", help="the size and write calls alone (profiling runs)")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "bench_csv_write.txt"))
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
        src = os.path.join(where, "bench_%d.csv" % rows)
        generate(src, rows)
        t = Table.from_csv(src, device=dev.index)
        os.remove(src)
        cols = [c.native() for c in t.columns.values()]
        line("table: %d rows x %d columns, %s" % (rows, len(cols), dict(t.schema)))
        held = {}
        row_start = torch.empty(rows + 1, dtype=torch.int64, device=dev)

        def size():
            held["total"] = ctx.csv_write_size(cols, rows, row_start.data_ptr())

        ms_size = best_ms(size, args.warmup, args.reps)
        total = held["total"]
        out = torch.empty(total, dtype=torch.uint8, device=dev)

        def write():
            ctx.csv_write_body(cols, rows, row_start.data_ptr(), out.data_ptr(), total)

        ms_write = best_ms(write, args.warmup, args.reps)
        both = ms_size + ms_write
        line("body: %d bytes (%.1f B/row)" % (total, total / rows))
        line("size: %.2f ms; write: %.2f ms; together %.2f ms, %.2f Mrows/s, %.2f GB/s of body bytes = %.2f %% of the "
             "%.2f TB/s copy ceiling" % (ms_size, ms_write, both, rows / both / 1e3, total / both / 1e6,
                                        100 * total / (both / 1e3) / COPY_CEILING, COPY_CEILING / 1e12))
        if args.device_only:
            continue

        def download():
            held["host"] = out.cpu().numpy()

        ms = best_ms(download, args.warmup, args.reps)
        line("download: %.2f ms, %.1f GB/s" % (ms, total / ms / 1e6))
        dst = os.path.join(where, "written_%d.csv" % rows)

        def to_file():
            held["host"].tofile(dst)

        ms = best_ms(to_file, args.warmup, args.reps)
        line("file write: %.2f ms, %.1f GB/s" % (ms, total / ms / 1e6))

        def whole():
            held["n"] = t.to_csv(dst)

        ms = best_ms(whole, args.warmup, args.reps)
        line("to_csv(path) whole: %.2f ms, %.2f Mrows/s (%d bytes with the header)" % (ms, rows / ms / 1e3, held["n"]))

        # yardstick: the device reader over the written file
        raw = np.fromfile(dst, dtype=np.uint8)
        data = torch.from_numpy(raw).to(dev)
        names = T._csv_first_record(raw[:1 << 16].tobytes())[0]

        def parse():
            handle, res, reports = ctx.csv_index(data.data_ptr(), len(raw), len(names), 1)
            assert not res.refusal_kind and res.nrows == rows
            keep = []
            try:
                for j, rep in enumerate(reports):
                    ty = T._csv_type_of_classes(rep.classes)
                    val = torch.zeros((rows + 63) // 64 * 8, dtype=torch.uint8, device=dev) if rep.valid < rows else None
                    vp = val.data_ptr() if val is not None else None
                    if ty == T.N.TYPE_STRING:
                        off = torch.empty(rows + 1, dtype=torch.int32, device=dev)
                        nb = ctx.csv_column(handle, j, ty, None, vp, off.data_ptr())
                        vals = torch.empty(nb + 16, dtype=torch.uint8, device=dev)
                        ctx.csv_column(handle, j, ty, vals.data_ptr(), None, off.data_ptr())
                        keep.append((vals, off, val))
                    else:
                        vals = torch.empty(rows * np.dtype(T.NUMPY_OF[ty]).itemsize, dtype=torch.uint8, device=dev)
                        ctx.csv_column(handle, j, ty, vals.data_ptr(), vp)
                        keep.append((vals, val))
            finally:
                ctx.csv_free(handle)

        ms = best_ms(parse, args.warmup, args.reps)
        line("yardstick, device reader's parse of the written file (bytes resident): %.2f ms, %.2f Mrows/s" % (ms, rows / ms / 1e3))
        del data, raw

        # yardstick: pyarrow's CSV writer after a download (Arrow's number formatting, not Java's)
        import pyarrow as pa
        import pyarrow.csv as pacsv

        def to_arrow():
            held["arrow"] = t.to_arrow()

        ms = best_ms(to_arrow, args.warmup, args.reps)
        line("yardstick, to_arrow() (download + wrap): %.2f ms" % ms)
        adst = os.path.join(where, "arrow_%d.csv" % rows)

        def arrow_write():
            pacsv.write_csv(held["arrow"], adst)

        ms = best_ms(arrow_write, args.warmup, args.reps)
        line("yardstick, pyarrow.csv.write_csv (%d threads; Arrow's formatting, %d bytes): %.2f ms, %.2f Mrows/s"
             % (pa.cpu_count(), os.path.getsize(adst), ms, rows / ms / 1e3))
        os.remove(adst)
        os.remove(dst)
        held.clear()
    line("csv write kernel launches: %r; routes: %r" % (ctx.csv_write_kernel_launches(), ctx.csv_write_routes()))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
