"""Cross-table checks on the GPU: dq_freq_probe and the functions over it against the plain-Python
model (tests/join_model.py). Every case compares the bitmap, the outcome bytes and `matched` with the model, exactly:
the outputs are bits, bytes and an integer count."""
import os
from decimal import Decimal

import numpy as np
import pytest

import deequ_amd as D
import deequ_amd.native as N
from deequ_amd import engine
from deequ_amd.groups import mix64
from deequ_amd.metrics import UnsupportedOnDevice
from deequ_amd.schema import _to_host
from deequ_amd.table import ChunkedTable, Table
import join_model as M

pytestmark = pytest.mark.gpu

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def _unmix64(z):
    """The inverse of groups.mix64 on one value (Python ints, mod 2^64)."""
    mask = (1 << 64) - 1

    def unxorshift(v, s):
        x = v
        for _ in range(64 // s + 1):
            x = v ^ (x >> s)
        return x
    z = unxorshift(z, 31)
    z = (z * pow(0x94D049BB133111EB, -1, 1 << 64)) & mask
    z = unxorshift(z, 27)
    z = (z * pow(0xBF58476D1CE4E5B9, -1, 1 << 64)) & mask
    return unxorshift(z, 30)


SENTINEL_U = _unmix64((1 << 64) - 1)
SENTINEL = SENTINEL_U - (1 << 64) if SENTINEL_U >> 63 else SENTINEL_U  # the LONG whose mixed key is the EMPTY marker


def test_the_side_counter_key_is_inverted_correctly():
    assert int(mix64(np.array([SENTINEL_U], dtype=np.uint64))[0]) == (1 << 64) - 1


def _table(data, types, device=True):
    t = Table.from_pydict(data, types=types)
    return t.to_device(0) if device else t


def _freq(table, cols):
    return engine.frequencies(Table([table[c] for c in dict.fromkeys(cols)]), list(cols))


def _probe_vs_model(rdata, rtypes, rcols, pdata, ptypes, pcols, device=True, ft=None):
    """Probe P against R's table: bitmap, outcome bytes and matched, each against the model. Returns the hits."""
    R, P = _table(rdata, rtypes, device), _table(pdata, ptypes, device)
    ft = ft or _freq(R, rcols)
    want = M.hits(M.rows_of(pdata, pcols), M.rows_of(rdata, rcols))
    n = len(want)
    matched, bits, out = ft.probe(P, pcols, want_bits=True, want_outcome=True)
    assert matched == sum(want)
    assert bits.cpu().numpy().tobytes()[:((n + 63) // 64) * 8] == M.bitmap(want)
    assert out.cpu().numpy()[:n].tolist() == [int(w) for w in want]
    only_count, b, o = ft.probe(P, pcols)
    assert only_count == matched and b is None and o is None
    return want


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _delta(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


# ---- 1. shapes ------------------------------------------------------------------------------------------------------
def _shape_data(np_, nr, kind):
    rng = np.random.default_rng(1000 * np_ + nr)
    hi = max(2 * nr, 4)

    def cell(v):
        return int(v) if kind == "long" else "k%d" % int(v)
    r = [None if rng.random() < 0.1 else cell(v) for v in rng.integers(0, hi, nr)]
    p = [None if rng.random() < 0.1 else cell(v) for v in rng.integers(0, hi, np_)]
    return {"r": r}, {"p": p}


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("kind", ["long", "string"])
@pytest.mark.parametrize("nr", [0, 1, 5, 3000])
@pytest.mark.parametrize("np_", [0, 1, 63, 64, 65, 4097])
def test_shapes_every_word_written_and_the_tail_clear(np_, nr, kind, device):
    """The output buffers start as 0xFF: every word and every byte is written, the bits past nrows are clear, and the
    guard word / guard bytes after them are untouched. P host-resident (staged for the call) and device-resident."""
    import torch
    rdata, pdata = _shape_data(np_, nr, kind)
    types = {"r": kind, "p": kind}
    R, P = _table(rdata, types, device), _table(pdata, types, device)
    ft = _freq(R, ["r"])
    want = M.hits(M.rows_of(pdata, ["p"]), M.rows_of(rdata, ["r"]))
    nb = ((np_ + 63) // 64) * 8
    bits = torch.full((nb + 8,), 0xFF, dtype=torch.uint8, device="cuda:0")
    out = torch.full((np_ + 8,), 0xFF, dtype=torch.uint8, device="cuda:0")
    matched = engine.ctx().freq_probe(ft.handle, [P["p"].native()], np_, [0], bits.data_ptr(), out.data_ptr())
    assert matched == sum(want)
    raw, cells = bits.cpu().numpy(), out.cpu().numpy()
    if np_:
        assert raw[:nb].tobytes() == M.bitmap(want) and cells[:np_].tolist() == [int(w) for w in want]
    assert (raw[nb:] == 0xFF).all() and (cells[np_:] == 0xFF).all()
    if np_ == 0:  # zero rows: DQ_OK, matched 0, nothing written
        assert (raw == 0xFF).all()


# ---- 2. fast path, LONG key ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["both", "p_only", "r_only"])
def test_fast_path_long_extremes_and_the_side_counter_key(where):
    base = [-1, -2, -(1 << 40), 0, 1, INT64_MIN, INT64_MAX, 12345678901234, None, 7, 7]
    r = base + ([SENTINEL] if where in ("both", "r_only") else [])
    p = [INT64_MIN, INT64_MAX, -1, -3, 0, 2, None, 7, INT64_MAX - 1, INT64_MIN + 1, -(1 << 40), 1 << 40] + \
        ([SENTINEL, SENTINEL] if where in ("both", "p_only") else []) + list(range(-40, 40))
    before = engine.ctx().freq_paths()
    want = _probe_vs_model({"r": r}, {"r": "long"}, ["r"], {"p": p}, {"p": "long"}, ["p"])
    assert _delta(before, engine.ctx().freq_paths()).get("small", 0) == 0  # one fixed-width key: no general build
    if where != "r_only":
        assert want[12] == want[13] == (where == "both")


# ---- 3. integer promotion ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptype, rtype, pvals, rvals", [
    ("int", "long", [-5, -1, 0, 7, -(1 << 31), (1 << 31) - 1, None, 100], [-1, -(1 << 31), 7, 1 << 31, (1 << 32) - 1, None, -5]),
    ("byte", "short", [-128, -1, 0, 127, 5, None, -7], [-1, 127, 255, -128, 128, 383, None, 5]),
    ("long", "byte", [-1, 255, 127, -128, 1 << 40, None], [-1, 127, -128]),
])
def test_integers_of_different_widths_compare_by_value(ptype, rtype, pvals, rvals):
    want = _probe_vs_model({"r": rvals}, {"r": rtype}, ["r"], {"p": pvals}, {"p": ptype}, ["p"])
    assert any(want) and not all(want)
    # and inside a two-column (general) key
    _probe_vs_model({"r": rvals, "s": ["x"] * len(rvals)}, {"r": rtype, "s": "string"}, ["r", "s"],
                    {"p": pvals, "q": ["x"] * len(pvals)}, {"p": ptype, "q": "string"}, ["p", "q"])


# ---- 4. NULLs ------------------------------------------------------------------------------------------------------
def test_null_never_matches_though_the_reference_holds_the_same_null():
    want = _probe_vs_model({"r": [1, None, None, 3]}, {"r": "long"}, ["r"], {"p": [None, 1, None, 2, 3]}, {"p": "long"},
                           ["p"])
    assert want == [False, True, False, False, True]
    rdata = {"a": [7, 7, None, None, 1], "b": [None, "x", "y", None, ""]}
    pdata = {"a": [7, 7, None, None, 1, 1, 7], "b": [None, "x", "y", None, "", None, "y"]}
    types = {"a": "long", "b": "string"}
    want = _probe_vs_model(rdata, types, ["a", "b"], pdata, types, ["a", "b"])
    assert want == [False, True, False, False, True, False, False]  # (7, NULL) does not hit R's (7, NULL)
    # R built under the grouping's include_nulls: its NULL rows are groups of the table and still never matched
    R = _table(rdata, types)
    ft = engine.frequencies(R, ["a", "b"], include_nulls=True)
    _probe_vs_model(rdata, types, ["a", "b"], pdata, types, ["a", "b"], ft=ft)


def test_null_in_a_compare_column_does_not_match():
    ds2 = _table({"id": [1, 2, 3, 4], "v": ["a", None, "c", "d"]}, {"id": "long", "v": "string"})
    ds1 = _table({"id": [1, 2, 3, 4], "v": ["a", None, None, "x"]}, {"id": "long", "v": "string"})
    res = D.DataSynchronization.columnMatch(ds1, ds2, {"id": "id"}, {"v": "v"}, assertion=lambda r: r == 0.25)
    assert res == D.ComparisonSucceeded(0.25)
    assert D.DataSynchronization.columnMatch(ds1, ds2, {"id": "id"}) == D.ComparisonSucceeded(1.0)


# ---- 5. strings ----------------------------------------------------------------------------------------------------
STRING_LENGTHS = [0, 1, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 40]


def _string_case():
    base = "abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGH"
    r = [base[:n] for n in STRING_LENGTHS] + ["日本語のキー", "ünïcødé", "ключ", None, "é" * 16 + "x"]
    p = list(r)
    for n in STRING_LENGTHS[1:]:
        p.append(base[:n - 1] + "#")  # the same length and prefix, the last byte differs
        p.append(base[:n] + "!")      # one byte longer
    p += ["", None, "日本語のキ一", "ünïcødè", "ключ", "é" * 16 + "y", "é" * 16, base]
    return r, p


@pytest.mark.parametrize("env, paths", [
    ({}, {"exact": 1, "small": 1}),
    ({"DQ_FREQ_NO_SMALL": "1"}, {"exact": 1, "sorted": 1}),
    ({"DQ_FREQ_NO_OPTIMISTIC": "1"}, {"exact": 1, "small": 1}),
])
def test_strings_by_length_and_bytes_on_every_general_build(env, paths):
    r, p = _string_case()
    rdata = {"r": r * 3}  # R holds every key three times: the representative is one of its rows
    R = _table(rdata, {"r": "string"})
    before = engine.ctx().freq_paths()
    with _env(**env):
        ft = _freq(R, ["r"])
    assert _delta(before, engine.ctx().freq_paths()) == paths
    want = _probe_vs_model(rdata, {"r": "string"}, ["r"], {"p": p}, {"p": "string"}, ["p"], ft=ft)
    assert sum(want) == len(r) - 1 + 2  # every non-NULL key of R once, plus the repeated "" and "ключ"
    assert want[p.index("")] and not want[p.index(None)]  # the empty string is a value, NULL is not


def test_strings_against_an_optimistically_built_table():
    """R of 2^22 rows takes the one-pass build without the sizing pass: representatives merged across workgroups."""
    import pyarrow as pa
    r, p = _string_case()
    words = np.array([w for w in r if w is not None], dtype=object)
    n = 1 << 22
    idx = (np.arange(n) * 7) % len(words)
    R = Table.from_arrow(pa.table({"r": pa.array(words[idx], type=pa.string())})).to_device(0)
    before = engine.ctx().freq_paths()
    ft = _freq(R, ["r"])
    assert _delta(before, engine.ctx().freq_paths()) == {"small": 1, "small_optimistic": 1}
    P = _table({"p": p}, {"p": "string"})
    want = M.hits(M.rows_of({"p": p}, ["p"]), [(w,) for w in words])
    matched, bits, out = ft.probe(P, ["p"], want_bits=True, want_outcome=True)
    assert matched == sum(want) and bits.cpu().numpy().tobytes()[:((len(p) + 63) // 64) * 8] == M.bitmap(want)
    assert out.cpu().numpy()[:len(p)].tolist() == [int(w) for w in want]


# ---- 6. fingerprint collisions -------------------------------------------------------------------------------------
def _narrowest_mask(R, cols):
    """The table of R under the narrowest fingerprint mask of 4 to 8 bits it still builds with (its distinct keys must
    keep distinct fingerprints), and the mask's bits."""
    for nbits in range(4, 9):
        with _env(DQ_FREQ_FP_MASK=hex((1 << nbits) - 1)):
            try:
                return _freq(R, cols), nbits
            except N.NativeError:
                continue
    raise AssertionError("no mask of 4 to 8 bits builds this table")


@pytest.mark.parametrize("shape", ["string", "long_string"])
def test_false_fingerprint_hits_are_rejected_by_the_comparison(shape):
    present = ["alpha", "beta " + "x" * 20, ""]
    absent = ["absent-%d" % i for i in range(50_000)]
    s = absent[:25_000] + present + absent[25_000:]
    if shape == "string":
        rdata, pdata, types, rc, pc = {"r": present * 2}, {"p": s}, {"r": "string", "p": "string"}, ["r"], ["p"]
    else:
        rdata = {"k": [5, 5, 6, 5, 5, 6], "r": present * 2}
        pdata = {"k": [5 + (i % 3 == 0) for i in range(len(s))], "p": s}
        types, rc, pc = {"k": "long", "r": "string", "p": "string"}, ["k", "r"], ["k", "p"]
    R = _table(rdata, types)
    ft, nbits = _narrowest_mask(R, rc)
    want = _probe_vs_model(rdata, types, rc, pdata, types, pc, ft=ft)
    # at most 2^8 fingerprints for 50 003 probe keys: thousands of them meet an equal fingerprint in the table
    assert nbits <= 8 and 0 < sum(want) <= 3


# ---- 7. R on the fast build ----------------------------------------------------------------------------------------
def test_probe_of_a_table_from_the_fast_build():
    """R: 2^24 + 5 distinct LONG keys 3 i - 1000 (the fast build's minimum). P: 1e6 rows drawn around R's range, so a
    third of the in-range values are keys; membership is arithmetic here, no set."""
    nr, np_ = (1 << 24) + 5, 1_000_000
    r = 3 * np.arange(nr, dtype=np.int64) - 1000
    rng = np.random.default_rng(5)
    p = rng.integers(-5000, 3 * nr + 5000, np_).astype(np.int64)
    p[:4] = [r[0], r[-1], r[-1] + 3, r[0] - 3]
    valid = rng.random(np_) > 0.01
    R = Table.from_arrays({"r": r}).to_device(0)
    P = Table.from_arrays({"p": p}, validity={"p": valid}).to_device(0)
    before = engine.ctx().freq_paths()
    ft = _freq(R, ["r"])
    assert _delta(before, engine.ctx().freq_paths()).get("fast_done", 0) == 1
    want = valid & ((p + 1000) % 3 == 0) & (p >= r[0]) & (p <= r[-1])
    matched, bits, out = ft.probe(P, ["p"], want_bits=True, want_outcome=True)
    assert matched == int(want.sum()) and 300_000 < matched < 340_000
    assert np.array_equal(np.unpackbits(bits.cpu().numpy(), bitorder="little", count=np_).astype(bool), want)
    assert np.array_equal(out.cpu().numpy()[:np_].astype(bool), want)


# ---- 8. self-probe -------------------------------------------------------------------------------------------------
def test_self_probe_hits_exactly_the_rows_without_a_null_component():
    rng = np.random.default_rng(8)
    n = 5000
    data = {"k": [None if rng.random() < 0.1 else int(v) for v in rng.integers(-50, 50, n)],
            "s": [None if rng.random() < 0.1 else "s%d" % v + "pad" * int(v % 7) for v in rng.integers(0, 40, n)],
            "d": [None if rng.random() < 0.1 else int(v) for v in rng.integers(17000, 17010, n)]}
    types = {"k": "long", "s": "string", "d": "date"}
    cols = ["k", "s", "d"]
    want = _probe_vs_model(data, types, cols, data, types, cols)
    assert want == [None not in row for row in M.rows_of(data, cols)] and 0 < sum(want) < n


# ---- 9. API --------------------------------------------------------------------------------------------------------
def _orders(device=True):
    data = {"oid": list(range(10)), "cid": [1, 2, 2, 3, None, 9, 1, 8, 3, 3]}
    return _table(data, {"oid": "long", "cid": "int"}, device), data


def _customers(device=True):
    data = {"id": [1, 2, 3, 4, None], "name": ["a", "b", "c", "d", "e"]}
    return _table(data, {"id": "long", "name": "string"}, device), data


def test_subset_check_ratio_and_assertion_both_ways():
    (orders, od), (customers, cd) = _orders(), _customers()
    ratio = M.matched(M.rows_of(od, ["cid"]), M.rows_of(cd, ["id"])) / 10
    assert ratio == 0.7
    assert D.ReferentialIntegrity.subsetCheck(orders, "cid", customers, "id", lambda v: v >= 0.7) == \
        D.ComparisonSucceeded(ratio)
    res = D.ReferentialIntegrity.subsetCheck(orders, ["cid"], customers, ["id"])  # default: is one
    assert isinstance(res, D.ComparisonFailed) and res.ratio == ratio and "0.7" in res.errorMessage
    assert D.ReferentialIntegrity.subsetCheck(customers, "id", customers, "id", lambda v: v == 0.8) == \
        D.ComparisonSucceeded(0.8)


@pytest.mark.parametrize("side", ["ds1", "ds2", "null_twice"])
def test_column_match_refuses_duplicate_keys_with_the_counts(side):
    a = {"id": [1, 2, 3, 4, None], "v": ["a", "b", "c", "d", "e"]}
    b = {"id": [1, 2, 3, 4, 5, 6], "v": ["a", "b", "c", "d", "e", "f"]}
    if side == "ds1":
        a["id"][3] = 1
    elif side == "ds2":
        b["id"][5] = 2
    else:
        a["id"][0] = None  # NULL is a key value under GROUP BY: two NULL keys are a duplicate
    types = {"id": "long", "v": "string"}
    ga, na = M.groups_and_rows(M.rows_of(a, ["id"]))
    gb, nb = M.groups_and_rows(M.rows_of(b, ["id"]))
    assert (ga, gb) != (na, nb)
    ds1, ds2 = _table(a, types), _table(b, types)
    for res in (D.DataSynchronization.columnMatch(ds1, ds2, {"id": "id"}, {"v": "v"}),
                D.DataSynchronization.columnMatchRowLevel(ds1, ds2, {"id": "id"})):
        assert isinstance(res, D.ComparisonFailed)
        assert "%d unique records and %d rows" % (ga, na) in res.errorMessage
        assert "%d unique records and %d rows" % (gb, nb) in res.errorMessage
    m = D.DatasetMatchAnalyzer(ds2, {"id": "id"}).calculate(ds1)
    assert m.value.isFailure and isinstance(m.value.failed, D.MetricCalculationRuntimeException)
    assert "%d unique records and %d rows" % (ga, na) in str(m.value.failed)


def _sync_case(n=3000):
    rng = np.random.default_rng(9)
    ids = rng.permutation(n * 2)[:n].tolist()
    v = ["v%d" % (i % 50) for i in range(n)]
    w = [int(x) for x in rng.integers(0, 5, n)]
    ds2 = {"key": ids, "val": v, "w": w}
    ds1 = {"id": list(ids), "value": list(v), "w": list(w)}
    for i in range(0, n, 7):
        ds1["value"][i] += "~"      # differs only in a compare column
    for i in range(3, n, 11):
        ds1["id"][i] = -1 - i       # a key absent from ds2
    for i in range(5, n, 13):
        ds1["w"][i] = None
    return ds1, {"id": "long", "value": "string", "w": "int"}, ds2, {"key": "int", "val": "string", "w": "long"}


def test_column_match_counts_the_rows_that_differ_only_in_a_compare_column():
    ds1, t1, ds2, t2 = _sync_case()
    A, B = _table(ds1, t1), _table(ds2, t2)
    n = len(ds1["id"])
    keys_only = M.matched(M.rows_of(ds1, ["id"]), M.rows_of(ds2, ["key"])) / n
    full = M.matched(M.rows_of(ds1, ["id", "value", "w"]), M.rows_of(ds2, ["key", "val", "w"])) / n
    assert full < keys_only < 1.0
    assert D.DataSynchronization.columnMatch(A, B, {"id": "key"}, assertion=lambda r: True) == D.ComparisonSucceeded(keys_only)
    res = D.DataSynchronization.columnMatch(A, B, {"id": "key"}, {"value": "val", "w": "w"}, assertion=lambda r: r > 0.5)
    assert res == D.ComparisonSucceeded(full)


def test_does_dataset_match_through_the_verification_suite():
    ds1, t1, ds2, t2 = _sync_case()
    A, B = _table(ds1, t1), _table(ds2, t2)
    n = len(ds1["id"])
    full = M.matched(M.rows_of(ds1, ["id", "value"]), M.rows_of(ds2, ["key", "val"])) / n
    good = D.Check(D.CheckLevel.Error, "in sync").doesDatasetMatch(B, {"id": "key"}, lambda r: r == full, {"value": "val"})
    bad = D.Check(D.CheckLevel.Warning, "fully in sync").doesDatasetMatch(B, {"id": "key"}, lambda r: r == 1.0,
                                                                         {"value": "val"}).hasSize(lambda s: s == n)
    result = D.VerificationSuite().onData(A).addCheck(good).addCheck(bad).run()
    assert result.status == D.CheckStatus.Warning
    assert result.checkResults[good].status == D.CheckStatus.Success
    assert [r.status for r in result.checkResults[bad].constraintResults] == \
        [D.ConstraintStatus.Failure, D.ConstraintStatus.Success]
    metric = result.metrics[D.DatasetMatchAnalyzer(B, {"id": "key"}, None, {"value": "val"})]
    assert metric.value.get() == full and (metric.name, metric.instance, metric.entity) == \
        ("DatasetMatch", "id", D.Entity.Dataset)


def test_two_halves_with_states_equal_the_whole_and_so_does_a_chunked_table():
    ds1, t1, ds2, t2 = _sync_case()
    B = _table(ds2, t2)
    n = len(ds1["id"])
    half = n // 2 + 3
    parts = [{c: v[:half] for c, v in ds1.items()}, {c: v[half:] for c, v in ds1.items()}]
    a = D.DatasetMatchAnalyzer(B, {"id": "key"}, None, {"value": "val"})
    want = M.matched(M.rows_of(ds1, ["id", "value"]), M.rows_of(ds2, ["key", "val"]))
    whole = D.AnalysisRunner.onData(_table(ds1, t1)).addAnalyzer(a).run().metric(a).value.get()
    assert whole == want / n
    first, both = D.InMemoryStateProvider(), D.InMemoryStateProvider()
    D.AnalysisRunner.onData(_table(parts[0], t1)).addAnalyzer(a).saveStatesWith(first).run()
    assert first.load(a) == D.DatasetMatchState(M.matched(M.rows_of(parts[0], ["id", "value"]),
                                                          M.rows_of(ds2, ["key", "val"])), half)
    ctx = D.AnalysisRunner.onData(_table(parts[1], t1)).addAnalyzer(a).aggregateWith(first).saveStatesWith(both).run()
    assert ctx.metric(a).value.get() == whole and both.load(a) == D.DatasetMatchState(want, n)
    chunked = ChunkedTable([_table(parts[0], t1), _table(parts[1], t1)])
    assert D.AnalysisRunner.onData(chunked).addAnalyzer(a).run().metric(a).value.get() == whole
    assert D.DataSynchronization.columnMatch(chunked, B, {"id": "key"}, {"value": "val"}, lambda r: True) == \
        D.ComparisonSucceeded(whole)
    assert D.ReferentialIntegrity.subsetCheck(chunked, "id", B, "key", lambda r: True).ratio == \
        M.matched(M.rows_of(ds1, ["id"]), M.rows_of(ds2, ["key"])) / n


def test_a_chunked_reference_is_refused():
    (orders, _), (customers, _) = _orders(), _customers()
    with pytest.raises(UnsupportedOnDevice, match="ChunkedTable"):
        D.ReferentialIntegrity.subsetCheck(orders, "cid", ChunkedTable([customers]), "id")


# ---- 10. row level -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [True, False])
def test_row_level_outcome_columns_equal_the_model(device):
    ds1, t1, ds2, t2 = _sync_case(1000)
    A, B = _table(ds1, t1, device), _table(ds2, t2, device)
    want_sync = M.hits(M.rows_of(ds1, ["id", "value"]), M.rows_of(ds2, ["key", "val"]))
    want_ref = M.hits(M.rows_of(ds1, ["id"]), M.rows_of(ds2, ["key"]))
    for out, want, name in ((D.DataSynchronization.columnMatchRowLevel(A, B, {"id": "key"}, {"value": "val"}), want_sync,
                             "outcome"),
                            (D.ReferentialIntegrity.subsetCheckRowLevel(A, "id", B, "key", "in_ref"), want_ref, "in_ref")):
        assert list(out.columns) == list(A.columns) + [name] and out.nrows == A.nrows
        col = out[name]
        assert col.spark_type == N.TYPE_BOOLEAN
        if device:
            assert col.values is None and col.device["values"].is_cuda  # stays in HBM
            col = _to_host(col)
        else:
            assert col.device is None
        assert col.values.tolist() == [int(w) for w in want] and col.validity is None
        for c in A.columns:
            assert out[c] is A[c]
    chunked = ChunkedTable([_table({c: v[:300] for c, v in ds1.items()}, t1, device),
                            _table({c: v[300:] for c, v in ds1.items()}, t1, device)])
    out = D.ReferentialIntegrity.subsetCheckRowLevel(chunked, "id", B, "key")
    assert isinstance(out, ChunkedTable) and [c.nrows for c in out.chunks] == [300, 700]
    cells = []
    for chunk in out.chunks:
        col = chunk["outcome"]
        cells += (_to_host(col) if device else col).values.tolist()
    assert cells == [int(w) for w in want_ref]


# ---- 11. launches --------------------------------------------------------------------------------------------------
def test_one_probe_launch_per_call_and_the_same_bits_twice():
    ds1, t1, ds2, t2 = _sync_case(2000)
    A, B = _table(ds1, t1), _table(ds2, t2)
    ctx = engine.ctx()
    for rc, pc in ((["key"], ["id"]), (["key", "val"], ["id", "value"])):
        ft = _freq(B, rc)
        before = ctx.kernel_launches()
        m1, b1, o1 = ft.probe(A, pc, want_bits=True, want_outcome=True)
        assert _delta(before, ctx.kernel_launches()) == {"freq_probe": 1}
        m2, b2, o2 = ft.probe(A, pc, want_bits=True, want_outcome=True)
        assert m1 == m2 and bool((b1 == b2).all()) and bool((o1 == o2).all())
        assert _delta(before, ctx.kernel_launches()) == {"freq_probe": 2}
    before = ctx.kernel_launches()
    D.ReferentialIntegrity.subsetCheck(A, "id", B, "key", lambda r: True)
    assert _delta(before, ctx.kernel_launches()) == {"freq_probe": 1}


def test_the_c_abi_refusals():
    (orders, _), (customers, _) = _orders(), _customers()
    ctx = engine.ctx()
    ft = _freq(customers, ["id"])
    cols = [orders["oid"].native(), orders["cid"].native()]
    with pytest.raises(N.NativeError, match="DQ_ERR_INVALID_ARGUMENT"):
        ctx.freq_probe(ft.handle, cols, 10, [0, 1])  # two probe keys, the table has one
    doubles = Table.from_arrays({"x": np.arange(10, dtype=np.float64)}).to_device(0)
    with pytest.raises(N.NativeError, match="DQ_ERR_UNSUPPORTED"):
        ctx.freq_probe(ft.handle, [doubles["x"].native()], 10, [0])
    names = _table({"name": ["a", None]}, {"name": "string"})
    hist = engine.frequencies(names, ["name"], include_nulls=True)  # counts NULL as "NullValue"
    with pytest.raises(N.NativeError, match="DQ_ERR_UNSUPPORTED"):
        ctx.freq_probe(hist.handle, [names["name"].native()], 2, [0])


# ---- 12. refusals fail alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptype, pvals, rtype, rvals", [
    ("double", [1.0, 2.0, 3.0], "double", [1.0, 2.0]),
    ("decimal(38,4)", [Decimal("1.5"), Decimal("2.5"), Decimal("3.5")], "decimal(38,4)", [Decimal("1.5")]),
    ("decimal", [Decimal("1.25"), Decimal("2.50"), Decimal("3.75")], "decimal", [Decimal("1.250"), Decimal("2.500")]),
])
def test_an_unsupported_pair_fails_alone(ptype, pvals, rtype, rvals):
    P = _table({"k": pvals, "id": [1, 2, 3]}, {"k": ptype, "id": "long"})
    R = _table({"k": rvals, "id": [1, 2][:len(rvals)]}, {"k": rtype, "id": "long"})
    bad = D.DatasetMatchAnalyzer(R, {"k": "k"})
    good = D.DatasetMatchAnalyzer(R, {"id": "id"})
    others = [D.Size(), D.Completeness("k"), D.Uniqueness(["id"]), D.Maximum("id")]
    alone = D.AnalysisRunner.onData(P).addAnalyzers(others).run()
    ctx = D.AnalysisRunner.onData(P).addAnalyzers([bad, good] + others).run()
    failed = ctx.metric(bad).value
    assert failed.isFailure and isinstance(failed.failed, UnsupportedOnDevice) and "column k" in str(failed.failed)
    assert ctx.metric(good).value.get() == len(rvals) / 3
    for a in others:
        assert ctx.metric(a).value.get() == alone.metric(a).value.get()
    assert isinstance(D.ReferentialIntegrity.subsetCheck(P, "k", R, "k"), D.ComparisonFailed)
