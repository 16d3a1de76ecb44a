#!/usr/bin/env python
"""One-GPU timing of the semi-join probe (not bench.py): dq_freq_probe alone (bitmap + count; the call returns after
its stream synchronised, so wall time is the time of the call), best of --reps after --warmup, next to the time
dq_frequencies takes to build a table over the same primary column in the same run, and next to numpy.isin on the
same arrays (its first --isin-rows primary rows against the whole reference) for the CPU line.
  LONG:   R = --ref-rows distinct int64 keys (C4's shape), P = --rows int64 rows, about half of them present.
  STRING: R = --str-ref-rows distinct 8-byte keys, P = --str-rows rows, about half present.
Prints ms, rows/s and the bytes of the traffic model; writes the same lines to --out."""
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


def long_column(torch, N, Column, name, values):
    c = Column(name, N.TYPE_LONG, None, None, length=values.numel())
    c.device = {"values": values}
    return c


def digit_strings(torch, N, Column, name, values, width=8, chunk=1 << 24):
    """Device STRING column of `values` (int64 tensor) as zero-padded decimal text of `width` bytes."""
    n = values.numel()
    data = torch.zeros(n * width + 16, dtype=torch.uint8, device=values.device)
    pow10 = torch.tensor([10 ** (width - 1 - k) for k in range(width)], dtype=torch.int64, device=values.device)
    for at in range(0, n, chunk):
        v = values[at:at + chunk]
        data[at * width:(at + v.numel()) * width] = ((v[:, None] // pow10[None, :]) % 10 + 48).to(torch.uint8).reshape(-1)
    c = Column(name, N.TYPE_STRING, None, None, length=n)
    c.device = {"values": data, "offsets": torch.arange(n + 1, dtype=torch.int64, device=values.device).mul_(width).to(torch.int32)}
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--ref-rows", type=int, default=100_000_000)
    ap.add_argument("--str-rows", type=int, default=250_000_000)
    ap.add_argument("--str-ref-rows", type=int, default=25_000_000)
    ap.add_argument("--isin-rows", type=int, default=100_000_000, help="primary rows numpy.isin takes (0: skip)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "bench_probe.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import deequ_amd.native as N
    from deequ_amd import engine
    from deequ_amd.table import Column, Table
    ctx = engine.ctx()
    dev = torch.device("cuda", engine.device())
    lines = []

    def line(txt):
        print(txt, flush=True)
        lines.append(txt)

    def case(label, np_, nr, make, per_row_bytes, general):
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        rvals = torch.arange(nr, dtype=torch.int64, device=dev).mul_(2)          # the even values: nr distinct keys
        pvals = torch.randint(0, 2 * nr, (np_,), dtype=torch.int64, device=dev, generator=gen)  # half of them even
        R, P = Table([make("r", rvals)]), Table([make("p", pvals)])
        torch.cuda.synchronize(dev)
        held = {}

        def build_ref():
            held.clear()
            held["t"] = engine.frequencies(R, ["r"])
        ref_ms = best_ms(build_ref, 0, 1)
        ft = held["t"]
        out = {}
        bits = torch.zeros((np_ + 63) // 64 * 8, dtype=torch.uint8, device=dev)
        pcols = [P["p"].native()]

        def probe():
            out["matched"] = ctx.freq_probe(ft.handle, pcols, np_, [0], bits.data_ptr())
        probe_ms = best_ms(probe, args.warmup, args.reps)
        matched = out["matched"]
        expect = int((pvals % 2 == 0).sum().item())
        if matched != expect:
            raise SystemExit("%s: probe matched %d rows, %d are present" % (label, matched, expect))
        del bits
        pb = {}

        def build_primary():
            pb.clear()
            pb["t"] = engine.frequencies(P, ["p"])
        build_ms = best_ms(build_primary, args.warmup, args.reps)
        pb.clear()
        # traffic model: the key bytes, one random 32-B table sector per row (general: + the 8-B representative index
        # and the reference row's cells), one output bit per row
        model = np_ * (per_row_bytes + 32 + (8 + per_row_bytes if general else 0)) + np_ / 8
        line("%s: R %d keys (table built in %.1f ms), P %d rows, %d matched" % (label, nr, ref_ms, np_, matched))
        line("%s: dq_freq_probe %.3f ms, %.2f Grows/s, model %.1f GB -> %.0f GB/s" %
             (label, probe_ms, np_ / probe_ms / 1e6, model / 1e9, model / probe_ms / 1e6))
        line("%s: dq_frequencies over the same P column %.3f ms, %.2f Grows/s (probe / build = %.2f)" %
             (label, build_ms, np_ / build_ms / 1e6, probe_ms / build_ms))
        if args.isin_rows and not general:
            k = min(args.isin_rows, np_)
            ph, rh = pvals[:k].cpu().numpy(), rvals.cpu().numpy()
            t0 = time.perf_counter()
            got = int(np.isin(ph, rh).sum())
            s = time.perf_counter() - t0
            if got != int((ph % 2 == 0).sum()):
                raise SystemExit("numpy.isin disagrees")
            line("%s: numpy.isin, the first %d P rows against all of R: %.1f s, %.4f Grows/s" % (label, k, s, k / s / 1e9))

    case("LONG", args.rows, args.ref_rows, lambda name, v: long_column(torch, N, Column, name, v), 8, False)
    # 8 key bytes + 4 offset bytes a row
    case("STRING", args.str_rows, args.str_ref_rows, lambda name, v: digit_strings(torch, N, Column, name, v), 12, True)
    line("kernel launches: %r" % {k: v for k, v in ctx.kernel_launches().items() if v})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
