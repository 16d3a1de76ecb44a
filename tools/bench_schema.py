#!/usr/bin/env python
"""One-GPU timing of RowLevelSchemaValidator on synthetic string columns (not bench.py).

Columns: DQ_SYNTH_STR_INT, DQ_SYNTH_STR_DEC, DQ_SYNTH_STR_TEXT and a generated "yyyy-MM-dd HH:mm:ss" column, 5 % NULLs
each. Three steps, each a child process under its own time limit (the parent never opens the GPU and stops at the first
step that fails):
  verdict   dq_schema_validate alone (4 definitions, one launch) between HIP events, against the sum of the existing
            passes that read the same bytes, measured in the same process: dq_cast_column(int column -> LONG), a
            MaxLength scan and a PatternMatch scan of the text column;
  attribute the verdict kernel over parts of the schema (one definition at a time, and all without the regex);
  validate  the whole RowLevelSchemaValidator.validate (verdict + compaction of both outputs), with the bytes the
            compaction moves.
Prints ms, rows/s and GB/s of bytes read; writes the same lines to --out.
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MASK = "yyyy-MM-dd HH:mm:ss"
TEXT_PATTERN = "^[a-z0-9 ]+$"


def build_table(rows):
    import torch
    import deequ_amd.native as N
    from deequ_amd import engine
    from deequ_amd.table import Column, Table
    ctx = engine.ctx()
    dev = torch.device("cuda", engine.device())
    cols = []

    def finish(name, data, off, seed):
        m = torch.zeros((rows + 63) // 64 * 8, dtype=torch.uint8, device=dev)
        ctx.synth_validity(seed, 0, rows, 50, m.data_ptr())
        c = Column(name, N.TYPE_STRING, None, None, length=rows)
        c.device = {"values": data, "offsets": off, "validity": m}
        cols.append(c)

    for j, (name, kind) in enumerate((("i", N.SYNTH_STR_INT), ("d", N.SYNTH_STR_DEC), ("s", N.SYNTH_STR_TEXT))):
        off = torch.empty(rows + 1, dtype=torch.int32, device=dev)
        total = ctx.synth_strings(kind, 0x5C4E0000 + j, 0, rows, off.data_ptr())
        data = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
        ctx.synth_strings(kind, 0x5C4E0000 + j, 0, rows, off.data_ptr(), data.data_ptr())
        finish(name, data, off, 0x5C4E0100 + j)
    # the timestamp column: 19 bytes per row, built in slices
    w = len(MASK)
    data = torch.zeros(rows * w + 16, dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(0x5C4E)
    step = 10_000_000
    for r0 in range(0, rows, step):
        m = min(step, rows - r0)

        def rnd(lo, hi):
            return torch.randint(lo, hi + 1, (m,), device=dev, generator=g, dtype=torch.int32)

        def dig(v, k):
            return ((v // 10 ** k) % 10 + 48).to(torch.uint8)

        def lit(ch):
            return torch.full((m,), ord(ch), dtype=torch.uint8, device=dev)

        y, mo, d, h, mi, s = rnd(1583, 9999), rnd(1, 12), rnd(1, 28), rnd(0, 23), rnd(0, 59), rnd(0, 59)
        parts = [dig(y, 3), dig(y, 2), dig(y, 1), dig(y, 0), lit("-"), dig(mo, 1), dig(mo, 0), lit("-"), dig(d, 1), dig(d, 0),
                 lit(" "), dig(h, 1), dig(h, 0), lit(":"), dig(mi, 1), dig(mi, 0), lit(":"), dig(s, 1), dig(s, 0)]
        data[r0 * w:(r0 + m) * w] = torch.stack(parts, dim=1).reshape(-1)
    off = (torch.arange(rows + 1, dtype=torch.int64, device=dev) * w).to(torch.int32)
    finish("t", data, off, 0x5C4E0103)
    torch.cuda.synchronize()
    ctx.synchronize()
    return Table(cols)


def build_schema():
    import deequ_amd as D
    return (D.RowLevelSchema().withIntColumn("i", minValue=-900000, maxValue=900000).withDecimalColumn("d", 10, 2)
            .withStringColumn("s", minLength=2, maxLength=18, matches=TEXT_PATTERN).withTimestampColumn("t", MASK))


def bytes_read(table):
    """Offsets + UTF-8 bytes + validity of every column."""
    n = table.nrows
    total = 0
    for c in table.columns.values():
        total += 4 * (n + 1) + (c.device["values"].numel() - 16) + (n + 7) // 8
    return total


class Timer:
    """HIP events on the stream the context runs on."""

    def __init__(self, torch, stream):
        self.torch, self.stream = torch, stream

    def ms(self, fn, warmup, reps):
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


def setup():
    import torch
    from deequ_amd import engine
    ctx = engine.ctx()
    stream = torch.cuda.Stream(device=engine.device())
    ctx.set_stream(stream.cuda_stream)  # the context's launches go to a stream torch can record events on
    return torch, ctx, stream


def line(out, label, ms, rows, nbytes=None):
    txt = "%-44s %10.3f ms  %8.1f Mrows/s" % (label, ms, rows / ms / 1e3)
    if nbytes is not None:
        txt += "  %8.1f GB/s" % (nbytes / ms / 1e6)
    print(txt, flush=True)
    out.append(txt)


def native_defs(torch, dev, names, schema, rows):
    """The dq_schema_column array of a schema with its cast buffers (and what must stay alive)."""
    import ctypes
    import deequ_amd.native as N
    nb = (rows + 63) // 64 * 8
    defs, keep = [], []
    for d in schema.columnDefinitions:
        sc = N.DqSchemaColumn()
        sc.kind, sc.column, sc.nullable = d.kind, names.index(d.name), 1
        prog = d.program()
        if prog:
            buf = ctypes.create_string_buffer(prog, len(prog))
            keep.append(buf)
            sc.program, sc.program_len = ctypes.addressof(buf), len(prog)
        if d.kind == N.SCHEMA_STRING:
            if d.minLength is not None:
                sc.has_min, sc.min_value = 1, d.minLength
            if d.maxLength is not None:
                sc.has_max, sc.max_value = 1, d.maxLength
        elif d.kind == N.SCHEMA_INT:
            sc.has_min, sc.min_value, sc.has_max, sc.max_value = 1, d.minValue, 1, d.maxValue
        if d.kind != N.SCHEMA_STRING:
            if d.kind == N.SCHEMA_DECIMAL:
                sc.precision, sc.scale = d.precision, d.scale
            vals = torch.zeros(rows, dtype=torch.int32 if d.kind == N.SCHEMA_INT else torch.int64, device=dev)
            mask = torch.zeros(nb, dtype=torch.uint8, device=dev)
            keep += [vals, mask]
            sc.cast_values, sc.cast_validity = vals.data_ptr(), mask.data_ptr()
        defs.append(sc)
    return defs, keep


def step_attribute(rows, warmup, reps):
    """The verdict kernel over parts of the schema: what each clause costs on its own."""
    import deequ_amd as D
    import deequ_amd.native as N
    torch, ctx, stream = setup()
    out = []
    with torch.cuda.stream(stream):
        t = build_table(rows)
        dev = t["i"].device["values"].device
        nb = (rows + 63) // 64 * 8
        bits = [torch.zeros(nb, dtype=torch.uint8, device=dev) for _ in range(3)]
        names = list(t.columns)
        cols = [t[c].native() for c in names]
        tm = Timer(torch, stream)
        R = D.RowLevelSchema
        variants = [
            ("int only", R().withIntColumn("i", minValue=-900000, maxValue=900000), ["i"]),
            ("decimal only", R().withDecimalColumn("d", 10, 2), ["d"]),
            ("timestamp only", R().withTimestampColumn("t", MASK), ["t"]),
            ("string lengths only", R().withStringColumn("s", minLength=2, maxLength=18), ["s"]),
            ("string regex only", R().withStringColumn("s", matches=TEXT_PATTERN), ["s"]),
            ("all but the regex", R().withIntColumn("i", minValue=-900000, maxValue=900000).withDecimalColumn("d", 10, 2)
             .withStringColumn("s", minLength=2, maxLength=18).withTimestampColumn("t", MASK), ["i", "d", "s", "t"]),
        ]
        for label, schema, read in variants:
            defs, keep = native_defs(torch, dev, names, schema, rows)

            def verdict():
                rc, _ = ctx.schema_validate(cols, rows, defs, N.SCHEMA_AMBIGUOUS_NULL, bits[0].data_ptr(),
                                            bits[1].data_ptr(), bits[2].data_ptr())
                ctx.check(rc, "dq_schema_validate")

            nbytes = bytes_read(Table_of(t, read))
            line(out, "verdict kernel: " + label, tm.ms(verdict, warmup, reps), rows, nbytes)
            del keep
    return out


def Table_of(t, names):
    from deequ_amd.table import Table
    return Table([t[n] for n in names])


def step_verdict(rows, warmup, reps):
    import deequ_amd as D
    import deequ_amd.native as N
    torch, ctx, stream = setup()
    with torch.cuda.stream(stream):
        t = build_table(rows)
        dev = t["i"].device["values"].device
        nb = (rows + 63) // 64 * 8
        bits = [torch.zeros(nb, dtype=torch.uint8, device=dev) for _ in range(3)]
        names = list(t.columns)
        defs, keep = native_defs(torch, dev, names, build_schema(), rows)
        cols = [t[c].native() for c in names]
        res = {}

        def verdict():
            rc, r = ctx.schema_validate(cols, rows, defs, N.SCHEMA_AMBIGUOUS_NULL, bits[0].data_ptr(), bits[1].data_ptr(),
                                        bits[2].data_ptr())
            ctx.check(rc, "dq_schema_validate")
            res["r"] = r

        tm = Timer(torch, stream)
        out = ["rows %d, bytes read by the verdict pass %d (%.2f B/row), warm-up %d, best of %d"
               % (rows, bytes_read(t), bytes_read(t) / rows, warmup, reps)]
        print(out[0], flush=True)
        line(out, "verdict kernel (4 definitions, 1 launch)", tm.ms(verdict, warmup, reps), rows, bytes_read(t))
        r = res["r"]
        out.append("  valid %d invalid %d unknown %d ambiguous %d" % (r.num_valid, r.num_invalid, r.num_unknown, r.num_ambiguous))
        print(out[-1], flush=True)
        # the existing passes over the same bytes, same process
        cv = torch.zeros(rows, dtype=torch.int64, device=dev)
        cm = torch.zeros(nb, dtype=torch.uint8, device=dev)
        icol = t["i"].native()
        t_cast = tm.ms(lambda: ctx.cast_column(icol, rows, N.TYPE_LONG, cv.data_ptr(), cm.data_ptr()), warmup, reps)
        line(out, "dq_cast_column(i -> LONG)", t_cast, rows)
        t_len = tm.ms(lambda: D.AnalysisRunner.onData(t).addAnalyzer(D.MaxLength("s")).run(), warmup, reps)
        line(out, "MaxLength(s) scan", t_len, rows)
        t_rx = tm.ms(lambda: D.AnalysisRunner.onData(t).addAnalyzer(D.PatternMatch("s", TEXT_PATTERN)).run(), warmup, reps)
        line(out, "PatternMatch(s) scan", t_rx, rows)
        line(out, "sum of the three existing passes", t_cast + t_len + t_rx, rows)
    return out


def step_validate(rows, warmup, reps):
    import deequ_amd as D
    torch, ctx, stream = setup()
    with torch.cuda.stream(stream):
        t = build_table(rows)
        schema = build_schema()
        res = {}

        def run():
            res["r"] = None  # release the previous outputs first
            res["r"] = D.RowLevelSchemaValidator.validate(t, schema, ambiguous="invalid")

        tm = Timer(torch, stream)
        t0 = time.perf_counter()
        ms = tm.ms(run, warmup, reps)
        wall = (time.perf_counter() - t0) * 1e3 / (warmup + reps)
        out = []
        line(out, "validate (verdict + both compactions)", ms, rows, bytes_read(t))
        r = res["r"]
        moved = 0
        for tab in (r.validRows, r.invalidRows):
            for c in tab.columns.values():
                moved += sum(v.numel() * v.element_size() for v in c.device.values())
        out.append("  valid %d invalid %d unknown %d ambiguous %d; compacted output %d bytes (%.2f B/row); "
                   "mean wall time per call %.1f ms" % (r.numValidRows, r.numInvalidRows, r.numUnknownRows,
                                                        r.numAmbiguousRows, moved, moved / rows, wall))
        print(out[-1], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schema", "bench_schema.txt"))
    ap.add_argument("--worker", choices=["verdict", "attribute", "validate"])
    args = ap.parse_args()
    if args.worker:
        fn = {"verdict": step_verdict, "attribute": step_attribute, "validate": step_validate}[args.worker]
        fn(args.rows, args.warmup, args.reps)
        return 0
    lines = []
    for step in ("verdict", "attribute", "validate"):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", step, "--rows", str(args.rows), "--warmup",
               str(args.warmup), "--reps", str(args.reps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print("step %s exceeded %d s: stopping" % (step, args.step_timeout))
            return 1
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            print("step %s failed (exit %d): stopping" % (step, p.returncode))
            return 1
        lines += p.stdout.splitlines()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
