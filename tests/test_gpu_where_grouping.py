"""`where` on the grouping analyzers and ApproxQuantile on the GPU: dq_filter_validity against numpy, and every
filtered metric against the oracle over a host table of the kept rows (`predicate_masks` for TRUE, then `frequencies`
/ `grouping_summary` / `group_counts_raw`). Counts, numRows and the ratios of counts are compared bit-exact, entropy and
MutualInformation within 1e-12 relative. Two identity checks compare the GPU with itself, as the specification words
them: the all-TRUE filter against the unfiltered analyzer, and the filtered ApproxQuantile against the unfiltered one
over the kept rows (both are exact order statistics)."""
import ctypes
import functools
import math

import numpy as np
import pytest

import deequ_amd as D
import deequ_amd.native as N
from deequ_amd import engine
from deequ_amd.table import DictColumn, PartedColumn, Table, pack_validity, unpack_validity
import oracle as O

pytestmark = pytest.mark.gpu

LONG_KEY = "a key well past fifteen bytes #"
W = "f > 0"  # NULL where f is NULL


def _close(a, b):
    return a == b or abs(a - b) <= 1e-12 * max(1.0, abs(b))


# ---- dq_filter_validity -------------------------------------------------------------------------------------------
def _raw_bitmap(mask, tail_ones):
    """pack_validity with the bits past len(mask) of the last 8-byte word set (an input the contract must ignore)."""
    bits = pack_validity(mask).copy()
    if tail_ones and len(bits):
        n = len(mask)
        for b in range(n, len(bits) * 8):
            bits[b >> 3] |= np.uint8(1 << (b & 7))
    return bits


@pytest.mark.parametrize("device_table", [True, False])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4099])
def test_filter_validity_against_numpy(n, device_table):
    """Two targets, `a` with a bitmap and `b` without, neither read by the predicate; input bits past nrows set to 1;
    the predicate is NULL where f is NULL. Every output word is written (the buffers start as 0xFF), the tail is zero,
    nothing past the last word is touched, true_rows is the popcount of TRUE. Host columns take the staging path."""
    import torch
    rng = np.random.default_rng(n + 1)
    f = rng.integers(-5, 6, n).astype(np.int64)
    fvalid = rng.random(n) > 0.2
    avalid = rng.random(n) > 0.3
    t = Table.from_arrays({"a": rng.integers(0, 9, n).astype(np.int64), "f": f, "b": np.arange(n, dtype=np.int64)},
                          validity={"a": avalid, "f": fvalid})
    t["a"].validity = _raw_bitmap(avalid, True)
    t["f"].validity = _raw_bitmap(fvalid, True)
    if device_table:
        t.to_device(0)
        for c, m in (("a", avalid), ("f", fvalid)):  # to_device repacks: put the raw tails back
            t[c].device["validity"] = torch.from_numpy(_raw_bitmap(m, True)).to("cuda:0")
    true = (f > 0) & fvalid
    if n:
        assert np.array_equal(O.predicate_masks(t, W)[0], true) and not O.predicate_masks(t, W)[1][~fvalid].any()
    batch = D.ScanBatch(t)
    pred = batch.preds[batch.predicate(W)]
    nwords = (n + 63) // 64
    outs = [torch.full(((nwords + 1) * 8,), 0xFF, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    ctx = engine.ctx()
    before = ctx.kernel_launches()
    got = ctx.filter_validity(batch.native_columns(), n, pred.to_native(), [0, 2], [o.data_ptr() for o in outs])
    after = ctx.kernel_launches()
    assert got == int(true.sum())
    assert after["filter_validity"] - before["filter_validity"] == (1 if n else 0)
    assert sum(after[k] - before[k] for k in ("pred_simple", "pred_vm", "regex")) == (1 if n else 0)
    for o, want in zip(outs, (true & avalid, true)):
        raw = o.cpu().numpy()
        assert np.array_equal(raw[:nwords * 8], pack_validity(want)[:nwords * 8]), n  # words and their zeroed tail
        assert (raw[nwords * 8:] == 0xFF).all()  # the guard word after the last one


def test_filter_validity_rejects_what_it_cannot_do():
    import torch
    t = Table.from_arrays({"a": np.arange(10, dtype=np.int64)}).to_device(0)
    batch = D.ScanBatch(t)
    pred = batch.preds[batch.predicate("a > 3")]
    out = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    ctx = engine.ctx()
    with pytest.raises(N.NativeError, match="DQ_ERR_ALIGNMENT"):
        ctx.filter_validity(batch.native_columns(), 10, pred.to_native(), [0], [out.data_ptr() + 4])
    with pytest.raises(N.NativeError, match="DQ_ERR_INVALID_ARGUMENT"):
        ctx.filter_validity(batch.native_columns(), 10, pred.to_native(), [3], [out.data_ptr()])
    with pytest.raises(N.NativeError, match="DQ_ERR_UNSUPPORTED"):
        ctx.filter_validity(batch.native_columns(), 10, pred.to_native(), [0] * 33, [out.data_ptr()] * 33)
    assert ctx.filter_validity(batch.native_columns(), 10, pred.to_native(), [0], [out.data_ptr()]) == 6


# ---- the ~5000-row table ------------------------------------------------------------------------------------------
N_ROWS = 5003


@functools.lru_cache(maxsize=None)
def _data():
    """Columns as Python lists. Rows 0..5 are planted: key group A first on a dropped row (0) and again on a kept row
    (3); group B only on dropped rows (1: f <= 0, 2: f NULL); row 4 has every key NULL and is kept; row 5 is a kept row
    of another group."""
    rng = np.random.default_rng(17)
    n = N_ROWS
    words = ["", "a", "bb", "ü", LONG_KEY, LONG_KEY + "2", "NullValue"] + ["w%d" % i for i in range(40)]
    k = [None if rng.random() < 0.05 else int(v) for v in rng.integers(0, 300, n)]
    dvals = rng.integers(0, 120, n) / 4.0
    d = []
    for v in dvals:
        u = rng.random()
        d.append(None if u < 0.05 else float("nan") if u < 0.08 else -0.0 if u < 0.11 else 0.0 if u < 0.14 else float(v))
    s = [None if rng.random() < 0.06 else words[int(rng.integers(0, len(words)))] for _ in range(n)]
    i = [None if rng.random() < 0.1 else int(v) for v in rng.integers(0, 6, n)]
    f = [None if rng.random() < 0.15 else int(v) for v in rng.integers(-4, 5, n)]
    planted = [  # k, d, s, i, f
        (1000, 1000.5, "group A", 7, -1),
        (2000, 2000.5, "group B only dropped", 8, 0),
        (2000, 2000.5, "group B only dropped", 8, None),
        (1000, 1000.5, "group A", 7, 3),
        (None, None, None, None, 2),
        (1001, -0.0, "", 7, 1),
    ]
    for r, (pk, pd, ps, pi, pf) in enumerate(planted):
        k[r], d[r], s[r], i[r], f[r] = pk, pd, ps, pi, pf
    return {"k": k, "d": d, "s": s, "i": i, "f": f, "one": [1] * n, "g": [None] * n}


TYPES = {"k": "long", "d": "double", "s": "string", "i": "int", "f": "long", "one": "long", "g": "long"}


def _table(rows=slice(None)):
    return Table.from_pydict({c: v[rows] for c, v in _data().items()}, types=TYPES)


@functools.lru_cache(maxsize=None)
def _host():
    return _table()


@functools.lru_cache(maxsize=None)
def _dev():
    return _table().to_device(0)


@functools.lru_cache(maxsize=None)
def _kept(where):
    """The host table of exactly the rows on which `where` is TRUE (the oracle's predicate evaluation)."""
    true, _ = O.predicate_masks(_host(), where)
    return _host().select_rows(true)


def _analyzers(cols, where):
    out = [D.Uniqueness(cols, where), D.Distinctness(cols, where), D.UniqueValueRatio(cols, where),
           D.CountDistinct(cols, where)]
    if len(cols) == 1:
        out += [D.Entropy(cols[0], where), D.MutualInformation([cols[0], "i"], where)]
    else:
        out += [D.MutualInformation(cols, where)]
    return out


def _host_mutual_information(freq, total):
    """MutualInformation's host formula over joint frequencies (A/MutualInformation.scala:35-97)."""
    px, py = {}, {}
    for (a, b), c in freq.items():
        px[a] = px.get(a, 0) + c
        py[b] = py.get(b, 0) + c
    terms = [(c / total) * math.log((c / total) / ((px[a] / total) * (py[b] / total)))
             for (a, b), c in freq.items() if a is not None and b is not None]
    return math.fsum(terms) if terms else None


def _expected(a, kept):
    """The metric value over the host table of kept rows from the oracle's frequencies, or None (empty state)."""
    freq, nrows = O.frequencies(kept, a.groupingColumns())
    if isinstance(a, D.MutualInformation):
        return _host_mutual_information(freq, nrows) if freq else None
    s = O.grouping_summary(freq, nrows)
    if s["num_groups"] == 0:
        return 0.0 if isinstance(a, D.CountDistinct) else None
    return {D.Uniqueness: lambda: s["num_unique"] / nrows, D.Distinctness: lambda: s["num_groups"] / nrows,
            D.UniqueValueRatio: lambda: s["num_unique"] / s["num_groups"], D.CountDistinct: lambda: float(s["num_groups"]),
            D.Entropy: lambda: s["entropy"]}[type(a)]()


def _check(a, metric, kept):
    want = _expected(a, kept)
    if want is None:
        assert metric.value.isFailure, (a, metric)
        return
    got = metric.value.get()
    if isinstance(a, (D.Entropy, D.MutualInformation)):
        assert _close(got, want), (a, got, want)
    else:
        assert got == want, (a, got, want)


KEYS = [["k"], ["d"], ["s"], ["s", "i"]]


def test_the_planted_cases_are_there():
    true, notnull = O.predicate_masks(_host(), W)
    assert list(true[:6]) == [False, False, False, True, True, True] and not notnull[2]
    assert (~notnull).sum() > 100 and true.sum() > 1000 and (~true).sum() > 1000
    kept = _kept(W)
    for cols in KEYS:
        full, _ = O.frequencies(_host(), cols)
        freq, nrows = O.frequencies(kept, cols)
        dropped = [key for key in full if key not in freq]
        assert dropped and nrows < kept.nrows  # a group dropped entirely; the kept all-NULL row takes no part


@pytest.mark.parametrize("device_table", [True, False])
@pytest.mark.parametrize("cols", KEYS, ids=lambda c: "+".join(c))
def test_filtered_grouping_metrics_match_the_oracle(cols, device_table):
    t = _dev() if device_table else _host()
    kept = _kept(W)
    an = _analyzers(cols, W)
    ctx = D.AnalysisRunner.onData(t).addAnalyzers(an).run()
    for a in an:
        _check(a, ctx.metric(a), kept)
    # the state: numRows, and every exported key decoded through the filtered view (group A's first row is dropped)
    state = an[0].computeStateFrom(t)
    freq, nrows = O.frequencies(kept, cols)
    assert state.numRows == nrows
    got = {tuple(O._group_key(v) for v in key): c for key, c in state.as_dict().items()}
    assert got == freq
    assert state.frequencies.source.filtered_where == W
    planted = {"k": 1000, "d": 1000.5, "s": "group A", "i": 7}
    assert got[tuple(O._group_key(planted[c]) for c in cols)] == 1


@pytest.mark.parametrize("cols", KEYS, ids=lambda c: "+".join(c))
def test_all_true_all_false_and_all_null_filters(cols):
    t = _dev()
    zero = _table(slice(0, 0)).to_device(0)
    plain = _analyzers(cols, None)
    unfiltered = D.AnalysisRunner.onData(t).addAnalyzers(plain).run()
    empty = D.AnalysisRunner.onData(zero).addAnalyzers(plain).run()
    for where, want_ctx, kept in (("one = 1", unfiltered, _host()), ("one = 0", empty, None), ("g > 0", empty, None)):
        an = _analyzers(cols, where)
        got = D.AnalysisRunner.onData(t).addAnalyzers(an).run()
        for a, p in zip(an, plain):
            g, w = got.metric(a), want_ctx.metric(p)
            assert g.value.isSuccess == w.value.isSuccess, (a, g, w)
            if w.value.isSuccess:
                assert g.value.get() == w.value.get(), (a, g, w)  # bit for bit
            else:
                assert type(g.value.failed) is type(w.value.failed), (a, g, w)
            assert (g.name, g.instance, g.entity) == (w.name, w.instance, w.entity)
            _check(a, g, kept if kept is not None else _host().select_rows(np.zeros(N_ROWS, dtype=bool)))


def test_mutual_information_with_where_matches_the_host_formula():
    a = D.MutualInformation(["s", "k"], W)
    freq, nrows = O.frequencies(_kept(W), ["s", "k"])
    want = _host_mutual_information(freq, nrows)
    for t in (_dev(), _host()):
        got = a.calculate(t).value.get()
        assert _close(got, want), (got, want)
    assert not _close(D.MutualInformation(["s", "k"]).calculate(_dev()).value.get(), want)


# ---- the fast build -----------------------------------------------------------------------------------------------
def test_filtered_long_keys_take_the_fast_build():
    """2^24 + 77 LONG rows, about 1e6 distinct keys, `where f < 0` over a second column: one fast build that produced
    its table, counts equal to the C oracle's over the kept rows. At this size the oracle's per-row Python predicate
    would take minutes: TRUE is the same comparison in numpy (f has no NULLs), tied to the oracle on the first rows."""
    n = (1 << 24) + 77
    rng = np.random.default_rng(5)
    pool = rng.integers(-2 ** 63, 2 ** 63 - 1, 1_000_000, dtype=np.int64)
    k = pool[rng.integers(0, len(pool), n)]
    f = rng.integers(-100, 100, n).astype(np.int64)
    true = f < 0
    head = Table.from_arrays({"k": k[:2000], "f": f[:2000]})
    assert np.array_equal(O.predicate_masks(head, "f < 0")[0], true[:2000])
    t = Table.from_arrays({"k": k, "f": f}).to_device(0)
    ctx = engine.ctx()
    before = ctx.freq_paths()
    state = D.Uniqueness(["k"], "f < 0").computeStateFrom(t)
    after = ctx.freq_paths()
    assert after["fast_done"] - before["fast_done"] == 1, {p: after[p] - before[p] for p in after}
    keys, counts = state.frequencies.export_raw()
    order = np.argsort(keys.view(np.uint64), kind="stable")
    okeys, ocounts, onulls = O.group_counts_raw(N.TYPE_LONG, k[true], None, int(true.sum()))
    assert onulls == 0 and state.numRows == int(true.sum())
    assert np.array_equal(keys.view(np.uint64)[order], okeys) and np.array_equal(counts[order], ocounts)


# ---- ChunkedTable -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chunked():
    cut, end = 4099, 4099 + 3001
    chunks = [_table(slice(0, cut)).to_device(0), _table(slice(cut, end)).to_device(0)]
    return D.ChunkedTable(chunks), _table(slice(0, end))


def test_chunked_table_filters_each_chunk_in_place():
    ct, whole = _chunked()
    true, _ = O.predicate_masks(whole, W)
    kept = whole.select_rows(true)
    view = engine.FilterCache().view(ct, W, ["s", "i"]).grouping_view(["s", "i"])
    assert all(isinstance(view[c], PartedColumn) and len(view[c].parts) == 2 for c in ("s", "i"))  # read in place
    ft = engine.frequencies(view, ["s", "i"])
    freq, nrows = O.frequencies(kept, ["s", "i"])
    assert ft.num_rows == nrows
    assert {tuple(O._group_key(v) for v in key): c for key, c in ft.to_dict().items()} == freq
    an = _analyzers(["s", "i"], W) + _analyzers(["k"], W) + [D.ApproxQuantile("k", 0.5, where=W)]
    got = D.AnalysisRunner.onData(ct).addAnalyzers(an).run()
    for a in an[:-1]:
        _check(a, got.metric(a), kept)
    vals = sorted(v for v in kept["k"].to_pylist() if v is not None)
    assert got.metric(an[-1]).value.get() == D.ApproxQuantile("k", 0.5).calculate(kept).value.get()
    assert got.metric(an[-1]).value.get() in vals


# ---- dictionary-encoded key ---------------------------------------------------------------------------------------
def test_kept_dictionary_column_stays_on_the_dictionary_counts(monkeypatch):
    import pyarrow as pa
    monkeypatch.setenv("DQ_RUN_SERIAL", "1")  # every build on this thread's context, whose counters are read below
    d = _data()
    at = pa.table({"s": pa.array(d["s"], type=pa.string()).dictionary_encode(), "f": pa.array(d["f"], type=pa.int64())})
    kept_enc = Table.from_arrow(at, dictionaries="keep").to_device(0)
    assert isinstance(kept_enc["s"], DictColumn)
    an = _analyzers(["s"], W)[:5]
    ctx = engine.ctx()
    before = ctx.kernel_launches()
    got = D.AnalysisRunner.onData(kept_enc).addAnalyzers(an).run()
    after = ctx.kernel_launches()
    assert after["dict_counts"] - before["dict_counts"] == 1 and after["dict_decode"] == before["dict_decode"]
    decoded = D.AnalysisRunner.onData(_dev()).addAnalyzers(an).run()
    for a in an:
        _check(a, got.metric(a), _kept(W))
        assert got.metric(a).value.get() == decoded.metric(a).value.get() or \
            _close(got.metric(a).value.get(), decoded.metric(a).value.get())


# ---- ApproxQuantile -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("column", ["k", "d", "i"])
def test_filtered_approx_quantile_is_the_quantile_of_the_kept_rows(column):
    kept = _kept(W)
    for q in (0.0, 0.5, 0.9):
        want = D.ApproxQuantile(column, q).calculate(kept.to_device(0) if q == 0.5 else kept)
        for t in (_dev(), _host()):
            got = D.ApproxQuantile(column, q, where=W).calculate(t)
            assert got.value.isSuccess and want.value.isSuccess
            g, w = got.value.get(), want.value.get()
            assert g == w or (math.isnan(g) and math.isnan(w)), (column, q, g, w)  # bit for bit
    none = D.ApproxQuantile(column, 0.5, where="g > 0").calculate(_dev())
    assert none.value.isFailure and type(none.value.failed) is type(
        D.ApproxQuantile(column, 0.5).calculate(_table(slice(0, 0))).value.failed)


def test_quantile_requests_key_on_the_filter_and_go_out_in_one_call(monkeypatch):
    calls = []
    real = N.Context.quantile_summaries
    monkeypatch.setattr(N.Context, "quantile_summaries", lambda self, reqs: calls.append(len(reqs)) or real(self, reqs))
    an = [D.ApproxQuantile("k", 0.5), D.ApproxQuantile("k", 0.5, where=W), D.ApproxQuantile("k", 0.25, where=W),
          D.ApproxQuantile("k", 0.5, where="f < 0")]
    got = D.AnalysisRunner.onData(_dev()).addAnalyzers(an).run()
    assert calls == [3]  # (k, 0.01), (k, 0.01, W), (k, 0.01, f < 0)
    assert all(got.metric(a).value.isSuccess for a in an)
    assert got.metric(an[1]).value.get() == D.ApproxQuantile("k", 0.5).calculate(_kept(W)).value.get()


# ---- sharing ------------------------------------------------------------------------------------------------------
def test_one_table_per_columns_and_filter_one_predicate_pass_per_text(monkeypatch):
    monkeypatch.setenv("DQ_RUN_SERIAL", "1")  # every build on this thread's context, whose counters are read below
    ctx = engine.ctx()
    t = _dev()

    def run(an):
        fp, kl = ctx.freq_paths(), ctx.kernel_launches()
        res = D.AnalysisRunner.onData(t).addAnalyzers(an).run()
        fp2, kl2 = ctx.freq_paths(), ctx.kernel_launches()
        return (res, sum(fp2[p] - fp[p] for p in fp2),
                sum(kl2[k] - kl[k] for k in ("pred_simple", "pred_vm", "regex")), kl2["filter_validity"] - kl["filter_validity"])
    _, one_build, one_pred, one_mask = run([D.Uniqueness(["k"], W)])
    assert one_build >= 1 and (one_pred, one_mask) == (1, 1)
    an = [D.Uniqueness(["k"], W), D.Distinctness(["k"], W), D.Uniqueness(["k"], "f < 0"), D.Entropy("i", W)]
    res, builds, preds, masks = run(an[:3])
    assert builds == 2 * one_build  # (k, W) shared by two analyzers, (k, f < 0)
    assert (preds, masks) == (2, 2)  # one predicate pass and one mask launch per distinct text
    res, builds, preds, masks = run(an)
    assert builds == 3 * one_build and (preds, masks) == (2, 2)  # W masks k and i in its one launch
    for a in an:
        _check(a, res.metric(a), _kept(a.where))
    assert res.metric(an[0]).value.get() != res.metric(an[2]).value.get()


# ---- states -------------------------------------------------------------------------------------------------------
def test_filtered_states_merge_and_persist(tmp_path):
    cut = 2777
    first, second = _table(slice(0, cut)).to_device(0), _table(slice(cut, None)).to_device(0)
    an = _analyzers(["s", "i"], W) + _analyzers(["k"], W)
    provider = D.InMemoryStateProvider()
    D.AnalysisRunner.onData(first).addAnalyzers(an).saveStatesWith(provider).run()
    merged = D.AnalysisRunner.onData(second).addAnalyzers(an).aggregateWith(provider).run()
    for a in an:
        _check(a, merged.metric(a), _kept(W))  # the filtered union
    schema = _host().schema
    p1, p2 = D.InMemoryStateProvider(), D.InMemoryStateProvider()
    D.AnalysisRunner.onData(first).addAnalyzers(an).saveStatesWith(p1).run()
    D.AnalysisRunner.onData(second).addAnalyzers(an).saveStatesWith(p2).run()
    again = D.AnalysisRunner.runOnAggregatedStates(schema, D.Analysis(an), [p1, p2])
    for a in an:
        _check(a, again.metric(a), _kept(W))
    # the filtered and the unfiltered Uniqueness side by side in one directory
    hdfs = D.HdfsStateProvider(None, str(tmp_path / "states"))
    plain, filtered = D.Uniqueness(["k"]), D.Uniqueness(["k"], W)
    D.AnalysisRunner.onData(_dev()).addAnalyzers([plain, filtered]).saveStatesWith(hdfs).run()
    back = D.HdfsStateProvider(None, str(tmp_path / "states"))
    for a, table in ((plain, _host()), (filtered, _kept(W))):
        state = back.load(a)
        freq, nrows = O.frequencies(table, ["k"])
        assert state is not None and state.numRows == nrows
        assert {tuple(O._group_key(v) for v in key): c for key, c in state.as_dict().items()} == freq
        _check(a, a.computeMetricFrom(state), table)


# ---- VerificationSuite and lone failures --------------------------------------------------------------------------
def test_is_unique_where_succeeds_where_is_unique_fails():
    t = Table.from_pydict({"id": [1, 2, 2, 3, None, 4], "active": [True, True, False, True, True, None]},
                          types={"id": "long", "active": "boolean"}).to_device(0)
    ok = D.Check(D.CheckLevel.Error, "filtered").isUnique("id").where("active")
    bad = D.Check(D.CheckLevel.Error, "unfiltered").isUnique("id")
    pk = D.Check(D.CheckLevel.Error, "pk").isPrimaryKey("id").where("active = true")
    res = D.VerificationSuite().onData(t).addCheck(ok).addCheck(bad).addCheck(pk).run()
    assert res.checkResults[ok].status == D.CheckStatus.Success
    assert res.checkResults[pk].status == D.CheckStatus.Success
    assert res.checkResults[bad].status == D.CheckStatus.Error
    assert res.metrics[D.Uniqueness(["id"], "active")].value.get() == 1.0
    assert res.metrics[D.Uniqueness(["id"])].value.get() == 3 / 5


def test_a_failing_where_fails_only_its_own_analyzer():
    t = _dev()
    missing, syntax = "nope > 1", "f >"
    an = [D.Uniqueness(["k"], missing), D.Entropy("k", syntax), D.ApproxQuantile("k", 0.5, where=missing),
          D.Uniqueness(["k"], W), D.Uniqueness(["k"]), D.ApproxQuantile("k", 0.5), D.Size(), D.Mean("k")]
    got = D.AnalysisRunner.onData(t).addAnalyzers(an).run()
    for a, text in ((an[0], missing), (an[1], syntax), (an[2], missing)):
        m, c = got.metric(a), D.Compliance("c", text).calculate(t)
        assert m.value.isFailure and c.value.isFailure
        assert type(m.value.failed) is type(c.value.failed) and str(m.value.failed) == str(c.value.failed)
    for a in an[3:]:
        assert got.metric(a).value.isSuccess, (a, got.metric(a))
    _check(an[3], got.metric(an[3]), _kept(W))
    _check(an[4], got.metric(an[4]), _host())
    # the same on a chunked table
    ct, whole = _chunked()
    got = D.AnalysisRunner.onData(ct).addAnalyzers(an).run()
    assert all(got.metric(a).value.isFailure for a in an[:3]) and all(got.metric(a).value.isSuccess for a in an[3:])
    # a 128-bit decimal column in the filter: the exception Compliance gives
    from decimal import Decimal
    wide = Table.from_pydict({"k": [1, 2, 2], "w": [Decimal(1), Decimal(2), None]},
                             types={"k": "long", "w": "decimal(38,0)"}).to_device(0)
    got = D.AnalysisRunner.onData(wide).addAnalyzers([D.Uniqueness(["k"], "w > 1"), D.Uniqueness(["k"])]).run()
    m, c = got.metric(D.Uniqueness(["k"], "w > 1")), D.Compliance("c", "w > 1").calculate(wide)
    assert m.value.isFailure and type(m.value.failed) is type(c.value.failed) and str(m.value.failed) == str(c.value.failed)
    assert got.metric(D.Uniqueness(["k"])).value.get() == 1 / 3
