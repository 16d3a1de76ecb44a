"""128-bit decimal columns (DQ_TYPE_DECIMAL128) on the GPU: the decimal128 scan kernel behind dq_scan (Completeness,
Sum, Mean, Minimum, Maximum, StandardDeviation, ApproxCountDistinct, each with an optional `where`), the wide source
of dq_cast_column, chunked tables, the reference's own decimal(38,18) known answer, mixed batches and the
ColumnProfiler. Expected values come from tests/decimal128_model.py. Bars: bit-exact for counts, sums, extremes,
HLL words and the casts; 1e-12 relative for the fp64 moments (README "Parity")."""
import functools
import math
from decimal import Decimal

import numpy as np
import pytest
import torch

import decimal128_model as M
import deequ_amd as D
from deequ_amd import engine
from deequ_amd import native as N
from deequ_amd.metrics import EmptyStateException, MetricCalculationRuntimeException, UnsupportedOnDevice
from deequ_amd.table import Column, Table, dec128_cells, pack_validity, unpack_validity

pytestmark = pytest.mark.gpu

TILE = N.DEC128_TILE_ROWS
SCALE = 18
SEVEN = ("Completeness", "Sum", "Mean", "Minimum", "Maximum", "StandardDeviation", "ApproxCountDistinct")


def analyzers(col="x", where=None):
    return {"Completeness": D.Completeness(col, where), "Sum": D.Sum(col, where), "Mean": D.Mean(col, where),
            "Minimum": D.Minimum(col, where), "Maximum": D.Maximum(col, where),
            "StandardDeviation": D.StandardDeviation(col, where),
            "ApproxCountDistinct": D.ApproxCountDistinct(col, where)}


@functools.lru_cache(maxsize=None)
def mixed_values(n, seed, null_fraction=0.05):
    """Fast-path cells (|v| < 2^53), long-division cells below and above 2^64 (the high limb of the latter is no
    sign extension), negatives of each, and NULLs. |v| < 2^105, so 10^5 rows sum below 10^38."""
    rnd = np.random.default_rng(seed)
    kind = rnd.integers(0, 4, n)
    out = []
    for i in range(n):
        if rnd.random() < null_fraction:
            out.append(None)
            continue
        k = int(kind[i])
        bits = (int(rnd.integers(1, 53)), int(rnd.integers(54, 64)), int(rnd.integers(65, 105)),
                int(rnd.integers(1, 105)))[k]
        v = int(rnd.integers(0, 1 << 62)) | (int(rnd.integers(0, 1 << 62)) << 62)
        v &= (1 << bits) - 1
        out.append(-v if rnd.random() < 0.5 else v)
    return tuple(out)


def wide_column(name, values, scale=SCALE, precision=38):
    mask = np.array([v is not None for v in values], dtype=bool)
    return Column(name, N.TYPE_DECIMAL128, dec128_cells([0 if v is None else v for v in values]),
                  None if mask.all() else pack_validity(mask), decimal_precision=precision, decimal_scale=scale)


def device_table(columns, trash=True):
    """The columns in HBM; with `trash`, every validity bit past the last row is set (the kernel must mask them)."""
    t = Table(columns).to_device(0)
    n = t.nrows
    for c in t.columns.values():
        v = c.device.get("validity")
        if trash and v is not None and n % 64:
            bits = unpack_validity(v.cpu().numpy(), len(v) * 8)
            bits[n:] = True
            c.device["validity"] = torch.from_numpy(np.packbits(bits, bitorder="little")).to(v.device)
    return t


def run(table, ans):
    provider = D.InMemoryStateProvider()
    res = D.AnalysisRunner.onData(table).addAnalyzers(list(ans)).saveStatesWith(provider).run()
    return res, provider


def check_against_model(values, res, provider, ans, scale=SCALE, kept=None):
    """The seven metrics of `ans` against the model over `values` (`kept`: the rows the `where` keeps; None = all,
    and then the Completeness denominator is every row)."""
    sel = list(values) if kept is None else [v for v, k in zip(values, kept) if k]
    want = M.metrics(sel, scale)
    nn = [v for v in sel if v is not None]
    for name in ("Sum", "Mean", "Minimum", "Maximum"):
        m = res.metric(ans[name])
        if want[name] is None:
            assert m.value.isFailure and isinstance(m.value.failed, EmptyStateException), (name, m)
        else:
            assert m.value.isSuccess, (name, m)
            assert M.bits(m.value.get()) == M.bits(want[name]), (name, m.value.get(), want[name])
    c = res.metric(ans["Completeness"])
    if len(sel) == 0:
        assert c.value.isFailure or math.isnan(c.value.get()), c
    else:
        assert c.value.get() == len(nn) / len(sel), c
    st = provider.load(ans["ApproxCountDistinct"])
    words = [w & ((1 << 64) - 1) for w in M.hll_words(nn)]
    assert st.words == words
    assert res.metric(ans["ApproxCountDistinct"]).value.get() == N.hll_count(words)
    sd = provider.load(ans["StandardDeviation"])
    if not nn:
        assert sd is None
    else:
        n, avg, m2 = want["moments"]
        assert sd.n == n
        if len(nn) <= 5000:  # the exact integer sums behind the state (order-free: any cut gives these)
            assert sd.sums == M.exact_sums(nn, scale)
            assert (sd.avg, sd.m2) == (avg, m2)  # the exact moments, rounded once
        assert abs(sd.avg - avg) <= 1e-12 * abs(avg) or avg == sd.avg, (sd.avg, avg)
        assert abs(sd.m2 - m2) <= 1e-12 * abs(m2), (sd.m2, m2)
        got = res.metric(ans["StandardDeviation"]).value.get()
        assert abs(got - math.sqrt(m2 / n)) <= 1e-12 * math.sqrt(m2 / n)


# ---- row counts: every path of the tile loop -------------------------------------------------------------------
@pytest.mark.parametrize("nrows", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 100_003])
def test_row_counts_with_nulls_and_trash_bits(nrows):
    values = mixed_values(nrows, 100 + nrows)
    if nrows >= 63:
        assert any(v is None for v in values)
    t = device_table([wide_column("x", values)])
    ans = analyzers()
    before = engine.ctx().kernel_launches()
    res, provider = run(t, ans.values())
    after = engine.ctx().kernel_launches()
    assert after["decimal128"] - before["decimal128"] == 1  # one launch for every wide slot of the call
    assert all(after[k] == before[k] for k in before if k != "decimal128")
    check_against_model(values, res, provider, ans)


def test_no_nulls_and_host_resident_column():
    values = mixed_values(5000, 7, null_fraction=0.0)
    ans = analyzers()
    for t in (device_table([wide_column("x", values)]), Table([wide_column("x", values)])):
        assert t["x"].validity is None
        res, provider = run(t, ans.values())
        check_against_model(values, res, provider, ans)
    host_nulls = mixed_values(3001, 8)
    res, provider = run(Table([wide_column("x", host_nulls)]), ans.values())
    check_against_model(host_nulls, res, provider, ans)


def test_all_null_column_has_no_states():
    values = (None,) * 1500
    ans = analyzers()
    res, provider = run(device_table([wide_column("x", values)]), ans.values())
    check_against_model(values, res, provider, ans)
    assert res.metric(ans["Completeness"]).value.get() == 0.0
    for name in ("Sum", "Mean", "Minimum", "Maximum", "StandardDeviation"):
        assert provider.load(ans[name]) is None


# ---- sums ------------------------------------------------------------------------------------------------------
def test_sum_whose_partials_pass_2_to_the_127():
    """First half +(10^38 - 1), second half -(10^38 - 1), plus a small remainder: every workgroup partial (and every
    lane's) leaves 128 bits while the total fits; the 192-bit accumulators and their fixed-order fold keep it exact."""
    big = M.LIMIT - 1
    half = 50_000
    values = [big] * half + [-big] * half + [12345678901234567890, -7, None, 3]
    t = device_table([wide_column("x", values)])
    ans = analyzers()
    res, provider = run(t, [ans["Sum"], ans["Mean"], ans["Minimum"], ans["Maximum"], ans["Completeness"]])
    total = 12345678901234567890 - 7 + 3
    assert provider.load(ans["Sum"]).wide == (total, SCALE)
    assert M.bits(res.metric(ans["Sum"]).value.get()) == M.bits(M.to_double(total, SCALE))
    assert M.bits(res.metric(ans["Mean"]).value.get()) == M.bits(M.to_double(total, SCALE) / (len(values) - 1))
    assert M.bits(res.metric(ans["Minimum"]).value.get()) == M.bits(M.to_double(-big, SCALE))
    assert M.bits(res.metric(ans["Maximum"]).value.get()) == M.bits(M.to_double(big, SCALE))
    assert res.metric(ans["Completeness"]).value.get() == (len(values) - 1) / len(values)


def test_overflowing_total_fails_sum_and_mean_alone():
    values = [9 * 10 ** 37] * 3
    ans = analyzers()
    res, _ = run(device_table([wide_column("x", values, scale=0)]), ans.values())
    for name in ("Sum", "Mean"):
        m = res.metric(ans[name])
        assert m.value.isFailure and isinstance(m.value.failed, MetricCalculationRuntimeException), m
        assert "overflow" in str(m.value.failed)
    assert res.metric(ans["Minimum"]).value.get() == 9e37 and res.metric(ans["Maximum"]).value.get() == 9e37
    assert res.metric(ans["Completeness"]).value.get() == 1.0
    assert res.metric(ans["StandardDeviation"]).value.get() == 0.0


# ---- where -----------------------------------------------------------------------------------------------------
def test_where_over_a_long_column_and_a_where_that_is_null_everywhere():
    n = 20_011
    values = mixed_values(n, 21)
    rnd = np.random.default_rng(5)
    k = [None if rnd.random() < 0.1 else int(v) for v in rnd.integers(-50, 50, n)]
    t = device_table([wide_column("x", values)] +
                     list(Table.from_pydict({"k": k, "z": [None] * n}, types={"k": "long", "z": "long"}).columns.values()))
    ans, plain = analyzers(where="k < 0"), analyzers()
    res, provider = run(t, list(ans.values()) + list(plain.values()) + [D.Size("k < 0"), D.Minimum("k")])
    kept = [kv is not None and kv < 0 for kv in k]
    sel = [v for v, keep in zip(values, kept) if keep]
    want = M.metrics(sel, SCALE)
    for name in ("Sum", "Mean", "Minimum", "Maximum"):
        assert M.bits(res.metric(ans[name]).value.get()) == M.bits(want[name]), name
    # Completeness(where): non-NULL rows under the filter over the rows the filter keeps
    assert res.metric(ans["Completeness"]).value.get() == len([v for v in sel if v is not None]) / sum(kept)
    assert provider.load(ans["ApproxCountDistinct"]).words == \
        [w & ((1 << 64) - 1) for w in M.hll_words(sel)]
    n_, avg, m2 = M.moments(sel, SCALE)
    sd = provider.load(ans["StandardDeviation"])
    assert sd.n == n_ and abs(sd.avg - avg) <= 1e-12 * abs(avg) and abs(sd.m2 - m2) <= 1e-12 * m2
    assert res.metric(D.Size("k < 0")).value.get() == sum(kept)
    check_against_model(values, res, provider, plain)  # the unfiltered slot of the same launch
    # a `where` that is NULL on every row: conditionalCount is NULL, no state anywhere
    nul = analyzers(where="z < 0")
    res, provider = run(t, nul.values())
    for name in ("Completeness", "Sum", "Mean", "Minimum", "Maximum", "StandardDeviation"):
        assert provider.load(nul[name]) is None, name
        assert res.metric(nul[name]).value.isFailure
    assert provider.load(nul["ApproxCountDistinct"]).words == [0] * 52


# ---- dq_cast_column: the per-row conversion, bit by bit ----------------------------------------------------------
def gpu_cast(values, scale, to_type, device):
    t = Table([wide_column("x", values, scale=scale)])
    if device:
        t.to_device(0)
    n = len(values)
    vals = torch.empty(max(n, 1), dtype=torch.float64 if to_type == N.TYPE_DOUBLE else torch.int64, device="cuda")
    mask = torch.zeros(max((n + 63) // 64, 1) * 8, dtype=torch.uint8, device="cuda")
    engine.ctx().cast_column(t["x"].native(), n, to_type, vals.data_ptr(), mask.data_ptr())
    return vals.cpu().numpy()[:n], unpack_validity(mask.cpu().numpy(), n)


def test_cast_to_double_and_long_bit_exact():
    by_scale = {}
    for v, s in M.hard_cases() + M.random_cases(4096, 99):
        by_scale.setdefault(s, []).append(v)
    assert len(by_scale) == 39
    for s, vs in sorted(by_scale.items()):
        vs = vs + [None]
        dv, ok = gpu_cast(vs, s, N.TYPE_DOUBLE, device=bool(s % 2))
        lv, ok2 = gpu_cast(vs, s, N.TYPE_LONG, device=not s % 2)
        assert list(ok) == [v is not None for v in vs] and list(ok2) == list(ok)
        for i, v in enumerate(vs[:-1]):
            assert M.bits(float(dv[i])) == M.bits(M.to_double(v, s)), (v, s, float(dv[i]))
            assert int(lv[i]) == M.to_long(v, s), (v, s, int(lv[i]))
        assert dv[-1] == 0.0 and lv[-1] == 0


# ---- chunking ---------------------------------------------------------------------------------------------------
CUTS = [0, 1, 64, 50_001, 100_003]


@functools.lru_cache(maxsize=None)
def whole_and_chunked():
    """One run over the whole table and one over the same rows as a ChunkedTable cut at rows 1, 64 and 50 001."""
    values = mixed_values(CUTS[-1], 31)
    ans = analyzers()
    whole, _ = run(device_table([wide_column("x", values)], trash=False), ans.values())
    chunks = D.ChunkedTable([device_table([wide_column("x", values[a:b])], trash=False)
                             for a, b in zip(CUTS, CUTS[1:])])
    got = D.AnalysisRunner.onData(chunks).addAnalyzers(list(ans.values())).run()
    return values, ans, whole, got


@pytest.mark.parametrize("name", [m for m in SEVEN if m != "StandardDeviation"])
def test_chunked_table_gives_the_whole_tables_bits(name):
    """Counts, the 192-bit sums, the extremes and the HLL registers are integers until the last step: any cut gives
    the bits of the whole table."""
    values, ans, whole, got = whole_and_chunked()
    w, g = whole.metric(ans[name]).value.get(), got.metric(ans[name]).value.get()
    print(name, repr(w), repr(g))
    assert M.bits(g) == M.bits(w), (name, g, w)
    if name in ("Sum", "Mean", "Minimum", "Maximum"):
        assert M.bits(g) == M.bits(M.metrics(list(values), SCALE)[name])


def test_chunked_table_gives_the_whole_tables_bits_standard_deviation():
    """The same bar for StandardDeviation: its state carries the exact integer sums of the per-row doubles and of
    their squares, which add exactly across lanes, workgroups and chunks; avg and m2 are rounded once from them. (fp64
    Chan merges alone differed by 1 ulp here: 1248213591816.9426 whole, ...9424 chunked.)"""
    _, ans, whole, got = whole_and_chunked()
    values, ans, whole, got = whole_and_chunked()
    w, g = whole.metric(ans["StandardDeviation"]).value.get(), got.metric(ans["StandardDeviation"]).value.get()
    print("StandardDeviation", repr(w), repr(g))
    assert M.bits(g) == M.bits(w), (g, w)
    assert M.bits(g) == M.bits(M.metrics(list(values), SCALE)["StandardDeviation"])


# ---- the reference's known answer ---------------------------------------------------------------------------------
def test_reference_kat_minimum_of_system_default_decimals():
    """T/analyzers/AnalyzerTests.scala:488-504: DecimalType.SYSTEM_DEFAULT = decimal(38,18), 123.45 / 99 / 678."""
    t = Table.from_rows([(Decimal("123.45"),), (Decimal("99"),), (Decimal("678"),)], ["att1"], ["decimal(38,18)"])
    assert t.schema["att1"] == "DecimalType(38,18)"
    for table in (t, device_table(list(t.columns.values()))):
        res = D.AnalysisRunner.onData(table).addAnalyzers([D.Minimum("att1"), D.Maximum("att1")]).run()
        assert res.metric(D.Minimum("att1")).value.get() == 99.0
        assert res.metric(D.Maximum("att1")).value.get() == 678.0
    check = D.Check(D.CheckLevel.Error, "wide").hasMin("att1", lambda v: v == 99.0).isComplete("att1") \
        .hasSum("att1", lambda v: v == 900.45)
    assert D.VerificationSuite().onData(t).addCheck(check).run().status == D.CheckStatus.Success


# ---- a mixed batch ------------------------------------------------------------------------------------------------
def test_mixed_batch_supported_metrics_and_lone_failures():
    n = 4099
    values = mixed_values(n, 41)
    rnd = np.random.default_rng(9)
    y = [None if rnd.random() < 0.1 else float(v) for v in rnd.normal(size=n)]
    s = ["s%d" % int(v) for v in rnd.integers(0, 40, n)]
    narrow = list(Table.from_pydict({"y": y, "s": s}, types={"y": "double", "s": "string"}).columns.values())
    t = device_table([wide_column("x", values)] + narrow)
    ans = analyzers()
    others = [D.Size(), D.Mean("y"), D.Maximum("y"), D.Completeness("y"), D.ApproxCountDistinct("s"), D.MaxLength("s"),
              D.Uniqueness(["s"])]
    failing = [D.Correlation("x", "y"), D.ApproxQuantile("x", 0.5), D.Uniqueness(["x"]), D.Histogram("x"),
               D.Compliance("pos", "x > 0"), D.PatternMatch("x", r"\d+"), D.KLLSketch("x"), D.Sum("y", "x > 1")]
    res, provider = run(t, list(ans.values()) + others + failing)
    check_against_model(values, res, provider, ans)
    for a in failing:
        m = res.metric(a)
        assert m.value.isFailure and isinstance(m.value.failed, UnsupportedOnDevice), (a, m)
    t2 = device_table(narrow)
    alone = D.AnalysisRunner.onData(t2).addAnalyzers(others).run()
    for a in others:
        assert res.metric(a).value.isSuccess and res.metric(a).value.get() == alone.metric(a).value.get(), a
    assert D.AnalysisRunner.onData(t2).addAnalyzers([D.Correlation("y", "y"), D.ApproxQuantile("y", 0.5)]).run() \
        .metric(D.ApproxQuantile("y", 0.5)).value.isSuccess
    # the launches of the batch without the wide column: what they are without this feature
    before = engine.ctx().kernel_launches()
    D.AnalysisRunner.onData(t2).addAnalyzers([a for a in others if not isinstance(a, D.Uniqueness)]).run()
    after = engine.ctx().kernel_launches()
    delta = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    assert delta == {"striped": 1, "strings": 1}, delta


# ---- ColumnProfiler ------------------------------------------------------------------------------------------------
def test_column_profiler_over_a_wide_column():
    values = mixed_values(3000, 51)
    t = device_table([wide_column("x", values)])
    p = D.ColumnProfiler.profile(t).profiles["x"]
    want = M.metrics(values, SCALE)
    nn = [v for v in values if v is not None]
    assert isinstance(p, D.NumericColumnProfile)
    assert p.dataType == D.DataTypeInstances.Fractional and not p.isDataTypeInferred and p.histogram is None
    assert p.completeness == want["Completeness"]
    assert p.approximateNumDistinctValues == int(N.hll_count([w & ((1 << 64) - 1) for w in M.hll_words(nn)]))
    # the reference profiles a decimal column through cast(DoubleType) (ColumnProfiler.scala:346-355): extremes are
    # the casts of the exact ones; sum, mean and stdDev run over the per-row doubles
    assert M.bits(p.minimum) == M.bits(want["Minimum"]) and M.bits(p.maximum) == M.bits(want["Maximum"])
    xs = [M.to_double(v, SCALE) for v in nn]
    assert abs(p.sum - math.fsum(xs)) <= 1e-12 * abs(math.fsum(xs))
    assert abs(p.mean - math.fsum(xs) / len(xs)) <= 1e-12 * abs(math.fsum(xs) / len(xs))
    assert abs(p.stdDev - want["StandardDeviation"]) <= 1e-12 * want["StandardDeviation"]
