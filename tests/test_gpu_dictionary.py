"""Dictionary-encoded string columns kept encoded on the GPU (`dictionaries="keep"`): dict_counts_kernel /
dict_fold_kernel / dq_dict_decode against the oracle over the decoded host table. Counts, lengths, HLL words and
DataType counts are compared bit-exact, entropy within 1e-12. DQ_DICT_LDS_ENTRIES=8 sends every dictionary of more
than 8 entries through the global-atomic path, so both counting paths run at small sizes."""
import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")

import deequ_amd as D
from deequ_amd import engine
from deequ_amd import native as N
from deequ_amd.table import DictColumn, Table
import oracle as O

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 63, 64, 65, 4099, 70_001]
DICT_SIZES = [1, 2, 64, 65, 1000]
# entries that classify as Integral / Fractional / Boolean / String, the empty string, multi-byte UTF-8, an e-mail
SPECIAL = ["a", "bb", "42", "-7", "3.14", "true", "false", "", "é中文", "😀x", "joe@example.com", "v12", " 7", "zzz"]


def entries_of(nd):
    """nd dictionary entries: the special ones first, then "e<k>"; with room for them a duplicate of entry 0 (entry 3)
    and a NULL entry (entry 2). The last entry of a dictionary of two or more is never indexed (unused)."""
    out = [(SPECIAL[i] if i < len(SPECIAL) else "e%d" % i) for i in range(nd)]
    if nd >= 4:
        out[2] = None
        out[3] = out[0]
    return out


def arrow_table(n, nd, null_rate, seed=0, hot=None):
    rng = np.random.default_rng(seed * 1000 + n + nd)
    usable = max(nd - 1, 1)
    idx = rng.integers(0, usable, n).astype(np.int32) if hot is None else np.full(n, hot, dtype=np.int32)
    mask = rng.random(n) < null_rate
    cat = pa.DictionaryArray.from_arrays(pa.array(idx, mask=mask), pa.array(entries_of(nd), type=pa.string()))
    k = pa.array(rng.integers(0, 10, n), mask=rng.random(n) < 0.05, type=pa.int64())
    knull = pa.array([None] * n, type=pa.int64())
    other = pa.array(np.array(["a", "bb", "q"], dtype=object)[rng.integers(0, 3, n)], type=pa.string())
    return pa.table({"cat": cat, "k": k, "knull": knull, "other": other})


def tables(n, nd, null_rate, seed=0, hot=None):
    """(kept device table, decoded host table for the oracle)."""
    at = arrow_table(n, nd, null_rate, seed, hot)
    kept = Table.from_arrow(at, dictionaries="keep")
    assert isinstance(kept["cat"], DictColumn)
    return kept.to_device(0), Table.from_arrow(at)


def run_states(t, analyzers):
    batch = D.ScanBatch(t)
    offs = [a.addOps(batch) for a in analyzers]
    res = batch.run()
    return [a.fromAggregationResult(res, o) for a, o in zip(analyzers, offs)]


def scan_analyzers(where):
    return [D.Completeness("cat", where), D.MinLength("cat", where), D.MaxLength("cat", where),
            D.ApproxCountDistinct("cat", where), D.DataType("cat", where),
            D.PatternMatch("cat", D.Patterns.EMAIL, where), D.PatternMatch("cat", r"^e\d+5$", where),
            D.Compliance("in", "cat IN ('a','bb')", where), D.Compliance("len", "length(cat) > 1", where),
            D.Compliance("null-safe", "cat IS NULL OR cat IN ('a','42')", where)]


def assert_states_equal(analyzers, got, dec):
    for a, g in zip(analyzers, got):
        exp = O.expected_state(dec, a)
        assert g == exp or (g is not None and exp is not None and repr(g) == repr(exp)), (a, g, exp)
        if isinstance(a, D.ApproxCountDistinct):
            assert [int(w) & 0xFFFFFFFFFFFFFFFF for w in g.words] == [int(w) & 0xFFFFFFFFFFFFFFFF for w in exp.words]


@pytest.mark.parametrize("nd", DICT_SIZES)
@pytest.mark.parametrize("n", ROWS)
def test_scan_states_match_oracle(n, nd, monkeypatch):
    """Every native scan op, without a where and under one over a LONG column, null rates 0 and 10 %, both counting
    paths: one dict_counts launch per call, no string scan, nothing decoded."""
    for null_rate in (0.0, 0.1):
        kept, dec = tables(n, nd, null_rate)
        analyzers = scan_analyzers(None) + scan_analyzers("k < 4")
        for lds in (None, "8"):
            if lds is None:
                monkeypatch.delenv("DQ_DICT_LDS_ENTRIES", raising=False)
            else:
                monkeypatch.setenv("DQ_DICT_LDS_ENTRIES", lds)
            before = engine.ctx().kernel_launches()
            got = run_states(kept, analyzers)
            after = engine.ctx().kernel_launches()
            assert after["dict_counts"] - before["dict_counts"] == 1
            assert after["strings"] == before["strings"] and after["dict_decode"] == before["dict_decode"]
            assert_states_equal(analyzers, got, dec)


def test_large_dictionary_at_the_default_threshold(monkeypatch):
    """About 20 000 entries: past the LDS threshold without the variable."""
    monkeypatch.delenv("DQ_DICT_LDS_ENTRIES", raising=False)
    kept, dec = tables(70_001, 20_011, 0.1, seed=3)
    analyzers = scan_analyzers(None)[:5] + [D.Compliance("len", "length(cat) > 4", "k < 4")]
    assert_states_equal(analyzers, run_states(kept, analyzers), dec)
    uniq, ent = D.Uniqueness(["cat"]), D.Entropy("cat")
    ctx = D.AnalysisRunner.onData(kept).addAnalyzers([uniq, ent]).run()
    freq, nrows = O.frequencies(dec, ["cat"])
    exp = O.grouping_summary(freq, nrows)
    assert ctx.metric(uniq).value.get() == exp["num_unique"] / nrows
    assert abs(ctx.metric(ent).value.get() - exp["entropy"]) <= 1e-12 * max(1.0, abs(exp["entropy"]))


@pytest.mark.parametrize("lds", [None, "8"])
def test_skew_all_rows_on_one_index(lds, monkeypatch):
    if lds:
        monkeypatch.setenv("DQ_DICT_LDS_ENTRIES", lds)
    else:
        monkeypatch.delenv("DQ_DICT_LDS_ENTRIES", raising=False)
    kept, dec = tables(70_001, 65, 0.1, seed=4, hot=10)
    analyzers = scan_analyzers(None) + scan_analyzers("k < 4")
    assert_states_equal(analyzers, run_states(kept, analyzers), dec)
    ctx = D.AnalysisRunner.onData(kept).addAnalyzers([D.CountDistinct(["cat"]), D.Entropy("cat")]).run()
    assert ctx.metric(D.CountDistinct(["cat"])).value.get() == 1.0
    assert ctx.metric(D.Entropy("cat")).value.get() == 0.0


def test_where_that_is_null_everywhere_and_all_null_column():
    kept, dec = tables(4099, 64, 0.1, seed=5)
    analyzers = scan_analyzers("knull > 0")
    assert_states_equal(analyzers, run_states(kept, analyzers), dec)
    # an all-NULL column: the states are absent (EmptyStateException), as over the decoded column
    at = pa.table({"cat": pa.DictionaryArray.from_arrays(pa.array([None] * 300, type=pa.int32()), pa.array(["a", "b"]))})
    kept, dec = Table.from_arrow(at, dictionaries="keep").to_device(0), Table.from_arrow(at)
    analyzers = [D.Completeness("cat"), D.MinLength("cat"), D.MaxLength("cat"), D.ApproxCountDistinct("cat"),
                 D.DataType("cat"), D.Compliance("in", "cat IN ('a')"), D.PatternMatch("cat", "a")]
    assert_states_equal(analyzers, run_states(kept, analyzers), dec)
    ctx = D.AnalysisRunner.onData(kept).addAnalyzers(
        [D.MinLength("cat"), D.Uniqueness(["cat"]), D.Entropy("cat"), D.Histogram("cat")]).run()
    assert isinstance(ctx.metric(D.MinLength("cat")).value.exception, D.EmptyStateException)
    want = D.AnalysisRunner.onData(dec).addAnalyzers([D.Uniqueness(["cat"]), D.Entropy("cat")]).run()
    for a in (D.Uniqueness(["cat"]), D.Entropy("cat")):
        assert ctx.metric(a).value.isSuccess == want.metric(a).value.isSuccess, a
    hist = ctx.metric(D.Histogram("cat")).value.get()
    assert {k: v.absolute for k, v in hist.values.items()} == {"NullValue": 300}


def test_checks_in_a_verification_suite():
    kept, dec = tables(4099, 65, 0.1, seed=6)
    check = (D.Check(D.CheckLevel.Error, "dictionary checks")
             .isContainedIn("cat", ["a", "bb", "42"], lambda v: v >= 0.0)
             .hasPattern("cat", r"^e\d+$", lambda v: v >= 0.0)
             .containsEmail("cat", lambda v: v >= 0.0)
             .isComplete("cat"))
    before = engine.ctx().kernel_launches()
    result = D.VerificationSuite().onData(kept).addCheck(check).run()
    after = engine.ctx().kernel_launches()
    assert after["dict_counts"] - before["dict_counts"] == 1 and after["strings"] == before["strings"]
    assert after["dict_decode"] == before["dict_decode"]
    assert len(result.metrics) == 4
    for a, m in result.metrics.items():
        exp = O.expected_state(dec, a).metricValue()
        assert m.value.get() == exp, (a, m.value.get(), exp)


@pytest.mark.parametrize("n,nd", [(0, 2), (1, 1), (65, 2), (4099, 64), (4099, 1000), (70_001, 65), (70_001, 1000)])
@pytest.mark.parametrize("lds", [None, "8"])
def test_grouping_analyzers_and_histogram_match_oracle(n, nd, lds, monkeypatch):
    if lds:
        monkeypatch.setenv("DQ_DICT_LDS_ENTRIES", lds)
    else:
        monkeypatch.delenv("DQ_DICT_LDS_ENTRIES", raising=False)
    kept, dec = tables(n, nd, 0.1, seed=7)
    an = [D.Uniqueness(["cat"]), D.Distinctness(["cat"]), D.UniqueValueRatio(["cat"]), D.CountDistinct(["cat"]),
          D.Entropy("cat"), D.Histogram("cat")]
    before = engine.ctx().kernel_launches()
    ctx = D.AnalysisRunner.onData(kept).addAnalyzers(an).run()
    after = engine.ctx().kernel_launches()
    assert after["dict_decode"] == before["dict_decode"] and after["dict_counts"] > before["dict_counts"]
    freq, nrows = O.frequencies(dec, ["cat"])
    exp = O.grouping_summary(freq, nrows)
    if nrows == 0:
        want = D.AnalysisRunner.onData(dec.to_device(0)).addAnalyzers(an[:5]).run()
        for a in an[:5]:
            assert ctx.metric(a).value.isSuccess == want.metric(a).value.isSuccess, a
    else:
        vals = {a: ctx.metric(a).value.get() for a in an[:5]}
        assert vals[an[0]] == exp["num_unique"] / nrows
        assert vals[an[1]] == exp["num_groups"] / nrows
        assert vals[an[2]] == exp["num_unique"] / exp["num_groups"]
        assert vals[an[3]] == float(exp["num_groups"])
        assert abs(vals[an[4]] - exp["entropy"]) <= 1e-12 * max(1.0, abs(exp["entropy"]))
    hfreq, hrows = O.frequencies(dec, ["cat"], include_nulls=True)
    hm = ctx.metric(an[5]).value
    if n == 0:
        return
    hist = hm.get()
    want = {("NullValue" if k[0] is None else k[0]): c for k, c in hfreq.items()}
    assert hist.numberOfBins == len(want)
    got = {k: v.absolute for k, v in hist.values.items()}
    assert got == want  # every detail count, the NullValue bin among them (at most 1000 bins here)
    for k, v in hist.values.items():
        assert v.ratio == want[k] / n


def test_entropy_fixed_point_sum_equals_the_decoded_run_bit_for_bit():
    kept, dec = tables(70_001, 1000, 0.1, seed=8)
    dec.to_device(0)
    a = D.Entropy("cat")
    got, want = a.computeStateFrom(kept).summary(), a.computeStateFrom(dec).summary()
    assert got["entropy_fx"] == want["entropy_fx"] and got["entropy"] == want["entropy"]
    assert (got["num_groups"], got["num_unique"]) == (want["num_groups"], want["num_unique"])


def test_launch_proof_and_what_still_decodes():
    kept, dec = tables(4099, 65, 0.1, seed=9)
    ctx = engine.ctx()
    # a batch without dictionary columns moves none of the three counters
    before = ctx.kernel_launches()
    run_states(kept, [D.Completeness("k"), D.Sum("k"), D.MaxLength("other")])
    after = ctx.kernel_launches()
    assert [after[k] - before[k] for k in ("dict_counts", "dict_fold", "dict_decode")] == [0, 0, 0]
    dec_dev = Table.from_arrow(arrow_table(4099, 65, 0.1, 9)).to_device(0)
    before = ctx.kernel_launches()
    run_states(dec_dev, scan_analyzers(None))
    after = ctx.kernel_launches()
    assert [after[k] - before[k] for k in ("dict_counts", "dict_fold", "dict_decode")] == [0, 0, 0]
    # a predicate that mixes the dictionary column with another column reads it decoded: one decode, cached
    mixed = [D.Compliance("eq", "cat = other"), D.Compliance("w", "k < 4", "cat = 'a'"), D.Completeness("cat")]
    before = ctx.kernel_launches()
    got = run_states(kept, mixed)
    after = ctx.kernel_launches()
    assert after["dict_decode"] - before["dict_decode"] == 1
    assert after["dict_counts"] - before["dict_counts"] == 1  # Completeness("cat") stays native in the same batch
    assert_states_equal(mixed, got, dec)
    # a two-column grouping and MutualInformation decode too (the cached column: no second decode)
    uniq, mi = D.Uniqueness(["cat", "other"]), D.MutualInformation(["cat", "other"])
    res = D.AnalysisRunner.onData(kept).addAnalyzers([uniq, mi]).run()
    freq, nrows = O.frequencies(dec, ["cat", "other"])
    exp = O.grouping_summary(freq, nrows)
    assert res.metric(uniq).value.get() == exp["num_unique"] / nrows
    want = D.AnalysisRunner.onData(dec_dev).addAnalyzers([mi]).run()
    assert abs(res.metric(mi).value.get() - want.metric(mi).value.get()) <= 1e-12
    assert ctx.kernel_launches()["dict_decode"] == after["dict_decode"]
    # a fresh kept table: the grouping alone decodes once
    kept2, _ = tables(4099, 65, 0.1, seed=9)
    before = ctx.kernel_launches()
    D.AnalysisRunner.onData(kept2).addAnalyzers([uniq]).run()
    assert ctx.kernel_launches()["dict_decode"] - before["dict_decode"] == 1


def test_device_decode_equals_the_host_decode():
    for n, nd in [(0, 1), (1, 2), (65, 64), (4099, 1000)]:
        kept, dec = tables(n, nd, 0.1, seed=10)
        col = kept["cat"].decoded()
        assert col.values is None and col.device is not None  # decoded in HBM
        got = [col.value_at(i) if col.valid_at(i) else None for i in range(n)] if n <= 65 else col.cells_at(np.arange(n))
        assert got == dec["cat"].to_pylist()
        total = int(col.device["offsets"][n].item())
        assert total == sum(len(s.encode()) for s in dec["cat"].to_pylist() if s is not None)
        assert col.device["values"].numel() == total + 16 and int(col.device["values"][total:].sum().item()) == 0


def test_bad_index_fails_the_call_and_is_never_an_address(monkeypatch):
    kept, _ = tables(4099, 64, 0.1, seed=11)
    col = kept["cat"]
    idx = col.indices.copy()
    valid = ~col.null_mask()
    rows = np.flatnonzero(valid)[[0, 100, 1000]]
    idx[rows] = [64, -1, 2 ** 31 - 1]  # built past the ingest check
    bad = DictColumn("cat", idx, col.validity, col.dictionary).to_device(0)
    t = Table([bad])
    for lds in ("8", "8192"):
        monkeypatch.setenv("DQ_DICT_LDS_ENTRIES", lds)
        with pytest.raises(N.NativeError, match="outside"):
            run_states(t, [D.Completeness("cat"), D.MaxLength("cat")])
    with pytest.raises(N.NativeError, match="outside"):
        bad.decoded()


def test_chunked_table_with_different_dictionaries():
    at = arrow_table(4099, 65, 0.1, seed=12)
    dec = Table.from_arrow(at)
    cut = 1500
    second = at.slice(cut)
    # the second chunk gets a dictionary of its own: the decoded values re-encoded
    second = second.set_column(0, "cat", second["cat"].combine_chunks().dictionary_decode().dictionary_encode())
    chunks = [Table.from_arrow(at.slice(0, cut), dictionaries="keep").to_device(0),
              Table.from_arrow(second, dictionaries="keep").to_device(0)]
    assert chunks[0]["cat"].dictionary.to_pylist() != chunks[1]["cat"].dictionary.to_pylist()
    ct = D.ChunkedTable(chunks)
    an = scan_analyzers(None)[:5] + [D.Uniqueness(["cat"]), D.CountDistinct(["cat"]), D.Entropy("cat"), D.Histogram("cat")]
    before = engine.ctx().kernel_launches()
    got = D.AnalysisRunner.onData(ct).addAnalyzers(an).run()
    for a in an[:5]:
        exp = O.expected_state(dec, a)
        g = got.metric(a).value.get()
        if isinstance(a, D.DataType):
            assert {k: v.absolute for k, v in g.values.items()} == \
                {"Unknown": exp.numNull, "Fractional": exp.numFractional, "Integral": exp.numIntegral,
                 "Boolean": exp.numBoolean, "String": exp.numString}
        else:
            want = O.hll_count(exp.words) if isinstance(a, D.ApproxCountDistinct) else exp.metricValue()
            assert g == want, (a, g, want)
    freq, nrows = O.frequencies(dec, ["cat"])
    exp = O.grouping_summary(freq, nrows)
    assert got.metric(an[5]).value.get() == exp["num_unique"] / nrows
    assert got.metric(an[6]).value.get() == float(exp["num_groups"])
    assert abs(got.metric(an[7]).value.get() - exp["entropy"]) <= 1e-12 * max(1.0, abs(exp["entropy"]))
    hfreq, _ = O.frequencies(dec, ["cat"], include_nulls=True)
    hist = got.metric(an[8]).value.get()
    assert {k: v.absolute for k, v in hist.values.items()} == \
        {("NullValue" if k[0] is None else k[0]): c for k, c in hfreq.items()}
    # helper contexts count their own launches; this thread's context never decoded
    assert engine.ctx().kernel_launches()["dict_decode"] == before["dict_decode"]


def test_persisted_grouping_state_merges_with_a_plain_table(tmp_path):
    at = arrow_table(4099, 65, 0.1, seed=13)
    kept = Table.from_arrow(at, dictionaries="keep").to_device(0)
    other_at = arrow_table(3001, 64, 0.1, seed=14)
    plain = Table.from_arrow(other_at).to_device(0)  # other rows, a plain string column
    prov = D.HdfsStateProvider(None, str(tmp_path / "s"))
    uniq, ent = D.Uniqueness(["cat"]), D.Entropy("cat")
    D.AnalysisRunner.onData(kept).addAnalyzers([uniq, ent]).saveStatesWith(prov).run()
    assert prov.load(uniq) is not None
    got = D.AnalysisRunner.onData(plain).addAnalyzers([uniq, ent]).aggregateWith(prov).run()
    union = Table.from_arrow(pa.concat_tables([pa.table({"cat": at["cat"].combine_chunks().dictionary_decode()}),
                                               pa.table({"cat": other_at["cat"].combine_chunks().dictionary_decode()})]))
    freq, nrows = O.frequencies(union, ["cat"])
    exp = O.grouping_summary(freq, nrows)
    assert got.metric(uniq).value.get() == exp["num_unique"] / nrows
    assert abs(got.metric(ent).value.get() - exp["entropy"]) <= 1e-12 * max(1.0, abs(exp["entropy"]))
    # and the other way round: a plain table's persisted state under a kept table's run
    prov2 = D.HdfsStateProvider(None, str(tmp_path / "s2"))
    D.AnalysisRunner.onData(plain).addAnalyzers([uniq]).saveStatesWith(prov2).run()
    got2 = D.AnalysisRunner.onData(kept).addAnalyzers([uniq]).aggregateWith(prov2).run()
    assert got2.metric(uniq).value.get() == exp["num_unique"] / nrows


def test_column_profiler_equals_the_oracle_profile_of_the_decoded_table():
    rng = np.random.default_rng(15)
    n = 4099

    def col(values):
        idx = rng.integers(0, len(values), n).astype(np.int32)
        return pa.DictionaryArray.from_arrays(pa.array(idx, mask=rng.random(n) < 0.1), pa.array(values))
    at = pa.table({"s_cat": col(["cat_%d" % i for i in range(50)]), "s_int": col([str(i * 37 - 500) for i in range(90)]),
                   "s_dec": col(["%.2f" % (i * 1.37) for i in range(200)]), "s_bool": col(["true", "false"]),
                   "x": pa.array(rng.normal(0, 1, n))})
    dec = Table.from_arrow(at)
    exp = O.expected_profile(dec)
    kept = Table.from_arrow(at, dictionaries="keep").to_device(0)
    assert all(isinstance(kept[c], DictColumn) for c in ("s_cat", "s_int", "s_dec", "s_bool"))
    prof = D.ColumnProfiler.profile(kept)
    assert prof.numRecords == n
    for name, e in exp.items():
        p = prof.profiles[name]
        assert p.completeness == e["completeness"], name
        assert p.approximateNumDistinctValues == e["approx_distinct"], name
        assert p.dataType == e["dataType"] and p.isDataTypeInferred == e["inferred"], name
        assert p.typeCounts == e["typeCounts"], name
        if e["dataType"] in ("Integral", "Fractional"):
            st = e["numeric"]
            assert (p.minimum, p.maximum) == (st["min"], st["max"]), name
            assert abs(p.mean - st["mean"]) <= 1e-12 * max(1.0, abs(st["mean"])), name
            assert abs(p.stdDev - st["stdDev"]) <= 1e-12 * max(1.0, abs(st["stdDev"])), name
        if e["histogram"] is None:
            assert p.histogram is None, name
        else:
            assert {k: v.absolute for k, v in p.histogram.values.items()} == e["histogram"], name
