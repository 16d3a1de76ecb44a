"""Row-level results on the GPU: dq_freq_row_bits against numpy, dq_row_outcomes against the numpy
model of the contract (tests/rowlevel_model.py, fed by the oracle), and VerificationResult.rowLevelResultsAsTable end
to end -- every check column row for row, the counts, the invariant that ties the rows to the metrics (matched /
considered is the metric, compared with ==), the compactions, and the table shapes. Everything is compared exactly:
the outputs are bits, bytes and integer counts."""
import functools

import numpy as np
import pytest

import deequ_amd as D
import deequ_amd.native as N
from deequ_amd import engine
from deequ_amd.metrics import UnsupportedOnDevice
from deequ_amd.schema import _to_host
from deequ_amd.table import ChunkedTable, DictColumn, Table, pack_validity, unpack_validity
import rowlevel_model as M

pytestmark = pytest.mark.gpu

LONG_KEY = "a key well past fifteen bytes #"
TILE = 4096  # rows of one wave tile of row_outcomes_kernel (rowlevel.hip kRowTileRows)
GRID_ROWS = 512 * 4 * TILE  # rows one pass of its largest grid covers (kRowMaxBlocks blocks of 4 waves)


def _raw_bitmap(mask, tail_ones=True):
    """pack_validity with the bits past len(mask) of the last 8-byte word set (an input the contracts must ignore)."""
    bits = pack_validity(mask).copy()
    if tail_ones:
        for b in range(len(mask), len(bits) * 8):
            bits[b >> 3] |= np.uint8(1 << (b & 7))
    return bits


def _words(n):
    return (n + 63) // 64


def _check_bitmap(tensor, want, n):
    """Every word holds `want` with a zeroed tail; the guard word after the last one is untouched (0xFF)."""
    raw = tensor.cpu().numpy()
    nb = _words(n) * 8
    assert np.array_equal(raw[:nb], pack_validity(want)[:nb]), n
    assert (raw[nb:] == 0xFF).all() and len(raw) == nb + 8


# ---- 1. dq_freq_row_bits -------------------------------------------------------------------------------------------
def _key_table(shape, n):
    rng = np.random.default_rng(100 + n)
    words = ["", "a", "bb", LONG_KEY, LONG_KEY + "2", "solo"] + ["w%d" % i for i in range(max(n // 3, 1))]
    k = [None if rng.random() < 0.15 else int(v) for v in rng.integers(0, max(n // 2, 2), n)]
    s = [None if rng.random() < 0.25 else words[int(rng.integers(0, len(words)))] for _ in range(n)]
    if n > 4:  # planted: NULL in one key only (rows 0, 1), NULL in both (row 2), a key seen once (row 3)
        k[0], s[0] = None, "a"
        k[1], s[1] = 5, None
        k[2], s[2] = None, None
        k[3], s[3] = 10 ** 12, "only once " + LONG_KEY
    cols = {"k": ["k"], "s": ["s"], "ks": ["k", "s"]}[shape]
    return Table.from_pydict({"k": k, "s": s}, types={"k": "long", "s": "string"}), cols, {"k": k, "s": s}


@pytest.mark.parametrize("shape", ["k", "s", "ks"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_freq_row_bits_against_numpy(n, shape):
    """unique == (group count == 1) & participates, part == some key non-NULL, both as FrequencyTable.row_counts() has
    them; every word written (the buffers start as 0xFF), tail bits zero, the guard word untouched."""
    import torch
    t, cols, data = _key_table(shape, n)
    t.to_device(0)
    keys = [tuple(data[c][i] for c in cols) for i in range(n)]
    part = np.array([any(v is not None for v in key) for key in keys], dtype=bool)
    seen = {}
    for key, p in zip(keys, part):
        if p:
            seen[key] = seen.get(key, 0) + 1
    unique = np.array([p and seen[key] == 1 for key, p in zip(keys, part)], dtype=bool)
    ft = engine.frequencies(Table([t[c] for c in cols]), cols)
    outs = [torch.full(((_words(n) + 1) * 8,), 0xFF, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    engine.ctx().freq_row_bits(ft.handle, outs[0].data_ptr(), outs[1].data_ptr(), n)
    _check_bitmap(outs[0], unique, n)
    _check_bitmap(outs[1], part, n)
    counts = ft.row_counts()
    assert np.array_equal(counts == 1, unique) and np.array_equal(counts > 0, part)


def test_freq_row_bits_rejects_what_row_counts_rejects():
    import torch
    t = Table.from_arrays({"k": np.arange(100, dtype=np.int64) % 7}).to_device(0)
    ft = engine.frequencies(t, ["k"])
    out = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    ctx = engine.ctx()
    with pytest.raises(N.NativeError, match="DQ_ERR_INVALID_ARGUMENT"):
        ctx.freq_row_bits(ft.handle, out.data_ptr(), out.data_ptr() + 16, 99)
    with pytest.raises(N.NativeError, match="DQ_ERR_ALIGNMENT"):
        ctx.freq_row_bits(ft.handle, out.data_ptr() + 4, out.data_ptr() + 16, 100)
    ctx.freq_row_bits(ft.handle, out.data_ptr(), out.data_ptr() + 16, 100)
    assert not out[:16].cpu().numpy().any()  # 100 rows over 7 keys: no row is unique
    assert np.array_equal(out[16:32].cpu().numpy(), pack_validity(np.ones(100, dtype=bool)))


# ---- 2. dq_row_outcomes --------------------------------------------------------------------------------------------
P_A, P_F, RX = "a >= 3", "f > 0", "^w1"
OUTCOME_TYPES = {"a": "long", "f": "long", "s": "string", "id": "long"}


@functools.lru_cache(maxsize=None)
def _outcome_case(n):
    """The host table of n rows, its raw validity masks, the BITS bitmaps and the model's six terms over three checks:
         check 0: a NOT NULL where `f > 0` (NULL where f is NULL) | `a >= 3` | id unique (BITS)
         check 1: s matches ^w1 where `a >= 3` (the predicate shared with check 0) | s NOT NULL
         check 2: `f > 0` alone"""
    rng = np.random.default_rng(n + 7)
    valid = {c: rng.random(n) > p for c, p in (("a", 0.3), ("f", 0.2), ("s", 0.1), ("id", 0.1))}
    a = rng.integers(0, 7, n).astype(np.int64)
    f = rng.integers(-3, 4, n).astype(np.int64)
    ids = rng.integers(0, max(n, 1), n).astype(np.int64)
    s = ["w%d" % v if ok else None for v, ok in zip(rng.integers(0, 30, n).tolist(), valid["s"].tolist())]
    data = {"a": [int(v) if ok else None for v, ok in zip(a, valid["a"])],
            "f": [int(v) if ok else None for v, ok in zip(f, valid["f"])], "s": s,
            "id": [int(v) if ok else None for v, ok in zip(ids, valid["id"])]}
    t = Table.from_pydict(data, types=OUTCOME_TYPES)
    uniq_ids, cnt = np.unique(ids[valid["id"]], return_counts=True)
    once = set(uniq_ids[cnt == 1].tolist())
    unique = np.array([ok and int(v) in once for v, ok in zip(ids, valid["id"])], dtype=bool)
    terms = [M.term_not_null(0, t, "a", P_F), M.term_predicate(0, t, P_A), (0, unique, valid["id"].copy()),
             M.term_pattern(1, t, "s", RX, P_A), M.term_not_null(1, t, "s"), M.term_predicate(2, t, P_F)]
    assert np.array_equal(M.term_unique(0, t, ["id"])[1], unique)  # the model's own uniqueness agrees with np.unique
    return data, valid, unique, terms


def _outcome_inputs(n, device_table):
    """A fresh table of the case with every validity bitmap's bits past nrows set to 1."""
    import torch
    data, valid, unique, terms = _outcome_case(n)
    t = Table.from_pydict(data, types=OUTCOME_TYPES)
    for c in t.columns:
        t[c].validity = _raw_bitmap(valid[c])
    if device_table:
        t.to_device(0)
        for c in t.columns:  # to_device repacks: put the raw tails back
            t[c].device["validity"] = torch.from_numpy(_raw_bitmap(valid[c])).to("cuda:0")
    bits = [torch.from_numpy(_raw_bitmap(m)).to("cuda:0") if n else torch.zeros(8, dtype=torch.uint8, device="cuda:0")
            for m in (unique, valid["id"])]
    return t, bits, terms


def _native_terms(batch, bits):
    pa_, pf, rx = batch.predicate(P_A), batch.predicate(P_F), batch.regex_predicate("s", RX)
    spec = [(N.ROW_NOT_NULL, batch.col_index["a"], pf, 0), (N.ROW_PREDICATE, pa_, -1, 0), (N.ROW_BITS, -1, -1, 0),
            (N.ROW_PREDICATE, rx, pa_, 1), (N.ROW_NOT_NULL, batch.col_index["s"], -1, 1), (N.ROW_PREDICATE, pf, -1, 2)]
    out = []
    for kind, index, where, check in spec:
        t = N.DqRowTerm()
        t.kind, t.index, t.where, t.check = kind, index, where, check
        if kind == N.ROW_BITS:
            t.pass_bits, t.considered_bits = bits[0].data_ptr(), bits[1].data_ptr()
        out.append(t)
    return out


def _check_buffers(n, null_mode, nchecks=3):
    import torch
    bufs, native = [], []
    for _ in range(nchecks):
        passed = torch.full(((_words(n) + 1) * 8,), 0xFF, dtype=torch.uint8, device="cuda:0")
        values = torch.full(((n + 15) // 16 * 16 + 16,), 0xFF, dtype=torch.uint8, device="cuda:0")
        validity = torch.full(((_words(n) + 1) * 8,), 0xFF, dtype=torch.uint8, device="cuda:0") if null_mode else None
        ck = N.DqRowCheck()
        ck.pass_bits, ck.values = passed.data_ptr(), values.data_ptr()
        ck.validity = validity.data_ptr() if null_mode else None
        bufs.append((passed, values, validity))
        native.append(ck)
    return bufs, native


def _check_outputs(bufs, outcomes, n, null_mode):
    pad = (n + 15) // 16 * 16
    for (passed, values, validity), want in zip(bufs, outcomes):
        _check_bitmap(passed, want.value, n)
        raw = values.cpu().numpy()
        assert np.array_equal(raw[:n], want.value.astype(np.uint8)), n
        assert (raw[n:pad] == 0).all()  # the padding up to 16 bytes is written as 0
        assert (raw[pad:] == 0xFF).all() and len(raw) == pad + 16  # the guard bytes are untouched
        if null_mode:
            _check_bitmap(validity, want.validity, n)


OUTCOME_SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 70001]  # the word, wave-tile and multi-block edges
PRED_KERNELS = ("pred_simple", "pred_vm", "regex")


def _run_outcomes(n, device_table, null_mode):
    """One dq_row_outcomes call of the six terms, then the same three distinct predicates as the Compliance ops of one
    dq_scan call: (term counts, check counts, output buffers, launch deltas of ours, launch deltas of the scan, the
    scan's states)."""
    t, bits, _ = _outcome_inputs(n, device_table)
    batch = D.ScanBatch(t)
    native_terms = _native_terms(batch, bits)
    preds = [p.to_native() for p in batch.preds]
    assert len(preds) == 3  # each distinct predicate once
    bufs, checks = _check_buffers(n, null_mode)
    ctx = engine.ctx()
    before = ctx.kernel_launches()
    tc, cc = ctx.row_outcomes(batch.native_columns(), n, preds, native_terms, checks,
                              N.ROW_FILTERED_NULL if null_mode else 0)
    after = ctx.kernel_launches()
    ops = []
    for p in range(3):
        op = N.DqOp()
        op.kind, op.where, op.predicate = N.OP_COMPLIANCE, -1, p
        op.column[0] = op.column[1] = -1
        ops.append(op)
    states = ctx.scan(batch.native_columns(), n, ops, preds)
    end = ctx.kernel_launches()
    ours = {k: after[k] - before[k] for k in after}
    scan = {k: end[k] - after[k] for k in end}
    return tc, cc, bufs, ours, scan, states


@pytest.mark.parametrize("null_mode", [False, True])
@pytest.mark.parametrize("device_table", [True, False])
@pytest.mark.parametrize("n", OUTCOME_SIZES)
def test_row_outcomes_against_model(n, device_table, null_mode):
    want_counts, outcomes = M.fold(_outcome_case(n)[3], 3, n, null_mode)
    tc, cc, bufs, ours, scan, states = _run_outcomes(n, device_table, null_mode)
    _check_outputs(bufs, outcomes, n, null_mode)
    assert tc == want_counts
    assert cc == [(o.true_rows, o.null_rows) for o in outcomes]
    assert all(o.true_rows + o.false_rows + o.null_rows == n for o in outcomes)
    assert ours["row_outcomes"] == (1 if n else 0)
    # three distinct predicates behind five uses (three terms, two filters): `a >= 3` and `f > 0` are evaluated by the
    # row_outcomes launch itself, the regex takes its one launch
    assert {k: ours[k] for k in PRED_KERNELS} == {"pred_simple": 0, "pred_vm": 0, "regex": 1 if n else 0}
    if n:  # and the terms without a `where` count what the scan's Compliance ops count
        assert states[0].u.num_matches_and_count.num_matches == tc[1][0]  # a >= 3
        assert states[1].u.num_matches_and_count.num_matches == tc[5][0]  # f > 0


@pytest.mark.parametrize("null_mode", [False, True])
@pytest.mark.parametrize("device_table", [True, False])
@pytest.mark.parametrize("n", OUTCOME_SIZES)
def test_row_outcomes_predicate_launches_against_scan(n, device_table, null_mode):
    """The predicate launches (pred_simple + pred_vm + regex) of the call against those of one dq_scan call with the
    same distinct predicates as Compliance ops, counted here. dq_scan evaluates `f > 0` and `a >= 3` -- `column <op>
    constant` over a numeric column -- inside a value-scan launch (fuse_compliance, scan_plan.cpp), which these three
    counters do not see; row_outcomes_kernel evaluates them itself, so both sides pay for the regex alone."""
    _, _, _, ours, scan, _ = _run_outcomes(n, device_table, null_mode)
    print("n=%d predicate launches: ours %s, dq_scan %s" % (n, {k: ours[k] for k in PRED_KERNELS},
                                                            {k: scan[k] for k in PRED_KERNELS}))
    assert sum(ours[k] for k in PRED_KERNELS) <= sum(scan[k] for k in PRED_KERNELS)


INLINE_PREDS = ["b > 1", "h <= -2", "i = 3", "l != 4", "fl >= 0.5", "d < 0.25", "3 <= l", "i > -1", "l > 2.5", "d >= 0",
                "fl = 1", "b >= 0", "h != 0", "i < 100", "l <= 0", "d > 1.5", "fl < 0", "b = 2", "h > 1"]


@pytest.mark.parametrize("device_table", [True, False])
def test_row_outcomes_inline_predicates_against_oracle(device_table):
    """`column <op> constant` predicates, which row_outcomes_kernel evaluates itself, over every fixed-width numeric
    type, with LONG and DOUBLE constants, a mirrored compare, a negated constant, NaN, -0.0 and NULLs, against the
    oracle's masks: 19 predicates, so the first 16 (kRowInline, rowlevel.hip) are inline and 3 take pred_simple launches.
    16 checks of one term, then three more terms in checks 0..2. n = 2 tiles and a partial one."""
    n = 2 * TILE + 405
    rng = np.random.default_rng(5)
    small = rng.integers(-4, 6, n)
    fl = rng.choice(np.array([-1.5, -0.0, 0.0, 0.5, 1.0, 2.0, np.nan], dtype=np.float32), n)
    d = rng.choice(np.array([-2.0, -0.0, 0.0, 0.25, 1.5, 3.0, np.nan]), n)
    arrays = {"b": small.astype(np.int8), "h": rng.permutation(small).astype(np.int16),
              "i": rng.integers(-2, 5, n).astype(np.int32), "l": rng.integers(-1, 6, n).astype(np.int64), "fl": fl, "d": d}
    t = Table.from_arrays(arrays, validity={c: rng.random(n) > 0.2 for c in arrays})
    terms = [M.term_predicate(k % 16, t, text) for k, text in enumerate(INLINE_PREDS)]
    want_counts, outcomes = M.fold(terms, 16, n, False)
    if device_table:
        t.to_device(0)
    batch = D.ScanBatch(t)
    native_terms = []
    for k, text in enumerate(INLINE_PREDS):
        tm = N.DqRowTerm()
        tm.kind, tm.index, tm.where, tm.check = N.ROW_PREDICATE, batch.predicate(text), -1, k % 16
        native_terms.append(tm)
    bufs, checks = _check_buffers(n, False, 16)
    ctx = engine.ctx()
    before = ctx.kernel_launches()
    tc, cc = ctx.row_outcomes(batch.native_columns(), n, [p.to_native() for p in batch.preds], native_terms, checks, 0)
    after = ctx.kernel_launches()
    assert tc == want_counts
    _check_outputs(bufs, outcomes, n, False)
    assert cc == [(o.true_rows, 0) for o in outcomes]
    assert {k: after[k] - before[k] for k in PRED_KERNELS} == {"pred_simple": 3, "pred_vm": 0, "regex": 0}
    assert after["row_outcomes"] - before["row_outcomes"] == 1


def test_row_outcomes_rejects_what_it_cannot_do():
    import torch
    t, bits, _ = _outcome_inputs(65, True)
    batch = D.ScanBatch(t)
    terms = _native_terms(batch, bits)
    preds = [p.to_native() for p in batch.preds]
    cols = batch.native_columns()
    bufs, checks = _check_buffers(65, True)
    ctx = engine.ctx()

    def call(terms=terms, checks=checks, flags=N.ROW_FILTERED_NULL):
        return ctx.row_outcomes(cols, 65, preds, terms, checks, flags)
    bad = _check_buffers(65, True)[1]
    bad[1].pass_bits += 4
    with pytest.raises(N.NativeError, match="DQ_ERR_ALIGNMENT"):
        call(checks=bad)
    bad = _check_buffers(65, True)[1]
    bad[0].values += 8
    with pytest.raises(N.NativeError, match="DQ_ERR_ALIGNMENT"):
        call(checks=bad)
    bad = _native_terms(batch, bits)
    bad[2].considered_bits += 4
    with pytest.raises(N.NativeError, match="DQ_ERR_ALIGNMENT"):
        call(terms=bad)
    bad = _native_terms(batch, bits)
    bad[0].index = len(cols)
    with pytest.raises(N.NativeError, match="DQ_ERR_INVALID_ARGUMENT"):
        call(terms=bad)
    bad = _native_terms(batch, bits)
    bad[1].index = len(preds)
    with pytest.raises(N.NativeError, match="DQ_ERR_INVALID_ARGUMENT"):
        call(terms=bad)
    with pytest.raises(N.NativeError, match="DQ_ERR_UNSUPPORTED"):
        call(terms=(terms * 11)[:65])
    with pytest.raises(N.NativeError, match="DQ_ERR_UNSUPPORTED"):
        call(checks=checks * 6)
    tc, _ = call()  # and the well-formed call still runs
    assert len(tc) == 6
    del bufs


# ---- 3. end to end -------------------------------------------------------------------------------------------------
N_ROWS = 5003
E2E_TYPES = {"id": "long", "k1": "long", "k2": "string", "s": "string", "v": "double", "f": "long"}
ALLOWED = ["w1", "w2", "w3", "", LONG_KEY]


@functools.lru_cache(maxsize=None)
def _e2e_data():
    rng = np.random.default_rng(23)
    n = N_ROWS
    words = ALLOWED + ["w%d" % i for i in range(4, 12)] + ["x9", "é"]

    def nullable(values, rate):
        return [None if rng.random() < rate else v for v in values]
    ids = rng.permutation(n).astype(np.int64)
    ids[rng.integers(0, n, 300)] = ids[rng.integers(0, n, 300)]  # some ids twice or more
    return {"id": nullable([int(v) for v in ids], 0.04),
            "k1": nullable([int(v) for v in rng.integers(0, 60, n)], 0.1),
            "k2": nullable([words[int(v)] for v in rng.integers(0, len(words), n)], 0.1),
            "s": nullable([words[int(v)] for v in rng.integers(0, len(words), n)], 0.08),
            "v": nullable([float(v) / 4 for v in rng.integers(-20, 200, n)], 0.07),
            "f": nullable([int(v) for v in rng.integers(-3, 4, n)], 0.15)}


def _e2e_table(rows=slice(None)):
    return Table.from_pydict({c: v[rows] for c, v in _e2e_data().items()}, types=E2E_TYPES)


def _e2e_checks():
    E = D.CheckLevel.Error
    a = (D.Check(E, "A").isComplete("v").isContainedIn("s", ALLOWED).hasPattern("s", r"^w[0-9]+$").where("f > 0")
         .hasSize(lambda v: v > 0))
    b = D.Check(E, "B").isUnique("id").isPrimaryKey("k1", "k2").where("f > 0").isNonNegative("v")
    c = D.Check(D.CheckLevel.Warning, "C").hasMean("v", lambda v: v > 0)
    return a, b, c


def _model_terms(check_index, check, host, chunked=False):
    """The model's terms of one check, built from its constraints' analyzers over the host table."""
    out = []
    for k in check.constraints:
        a = k.inner.analyzer
        if isinstance(a, D.Completeness):
            out.append(M.term_not_null(check_index, host, a.column, a.where))
        elif isinstance(a, D.PatternMatch):
            out.append(M.term_pattern(check_index, host, a.column, a.pattern, a.where))
        elif isinstance(a, D.Compliance):
            out.append(M.term_predicate(check_index, host, a.predicate, a.where))
        elif isinstance(a, (D.Uniqueness, D.UniqueValueRatio)) and not chunked:
            out.append(M.term_unique(check_index, host, a.columns, a.where))
    return out


@functools.lru_cache(maxsize=None)
def _e2e_model(null_mode):
    host = _e2e_table()
    a, b, _ = _e2e_checks()
    return M.fold(_model_terms(0, a, host) + _model_terms(1, b, host), 2, N_ROWS, null_mode)


@functools.lru_cache(maxsize=None)
def _e2e_run(device_table):
    t = _e2e_table()
    if device_table:
        t.to_device(0)
    checks = _e2e_checks()
    result = D.VerificationSuite().onData(t).addChecks(list(checks)).run()
    return t, checks, result


def _column_arrays(col, n):
    """(values as bool, validity as bool or None) of a BOOLEAN check column, device-only or host."""
    if col.values is None:
        col = _to_host(col)
    vals = np.asarray(col.values).view(np.uint8)[:n].astype(bool)
    return vals, (None if col.validity is None else unpack_validity(col.validity, n))


def _assert_columns(res, outcomes, names, n, null_mode):
    for name, want in zip(names, outcomes):
        col = res.table[res.checkColumns[name]]
        assert col.spark_type == N.TYPE_BOOLEAN and col.length == n
        vals, validity = _column_arrays(col, n)
        assert np.array_equal(vals, want.value), name
        if null_mode:
            assert np.array_equal(validity, want.validity), name
        else:
            assert validity is None
        assert (res.passedRows[name], res.failedRows[name], res.nullRows[name]) == \
            (want.true_rows, want.false_rows, want.null_rows)
        assert res.passedRows[name] + res.failedRows[name] + res.nullRows[name] == n


@pytest.mark.parametrize("filteredRow", ["true", "null"])
@pytest.mark.parametrize("device_table", [True, False])
def test_end_to_end_against_model(device_table, filteredRow):
    t, (a, b, c), result = _e2e_run(device_table)
    null_mode = filteredRow == "null"
    res = D.VerificationResult.rowLevelResultsAsTable(result, t, filteredRow=filteredRow)
    assert isinstance(res, D.RowLevelResults) and res.skipped == []
    assert list(res.checkColumns) == ["A", "B"] and "C" not in res.checkColumns  # hasMean has no row-level form
    assert list(res.table.columns) == list(t.columns) + ["A", "B"]
    assert (res.table["A"].device is not None) == device_table
    want_counts, outcomes = _e2e_model(null_mode)
    _assert_columns(res, outcomes, ["A", "B"], N_ROWS, null_mode)
    if null_mode:
        assert res.nullRows["A"] > 0 and res.nullRows["B"] > 0
    # one (matched, considered) per row-level constraint, in check and constraint order
    constraints = a.constraints[:3] + b.constraints
    assert [(d, k) for d, k, _, _ in res.termCounts] == [("A", k) for k in a.constraints[:3]] + [("B", k) for k in b.constraints]
    assert [(m, k) for _, _, m, k in res.termCounts] == want_counts
    # the invariant that ties the rows to the metrics: matched / considered IS the metric, and the analyzer's state
    for (_, constraint, matched, considered) in res.termCounts:
        analyzer = constraint.inner.analyzer
        if isinstance(analyzer, (D.Completeness, D.Compliance, D.PatternMatch)):
            assert matched / considered == result.metrics[analyzer].value.get(), constraint
            state = analyzer.computeStateFrom(t)
            assert (state.numMatches, state.count) == (matched, considered), constraint
    # isUnique("id"): the ids that occur once, counted directly
    ids = np.array([v for v in _e2e_data()["id"] if v is not None], dtype=np.int64)
    _, cnt = np.unique(ids, return_counts=True)
    _, _, matched, considered = res.termCounts[3]
    assert (matched, considered) == (int((cnt == 1).sum()), len(ids))
    # Uniqueness divides the groups of count 1 by numRows, the rows with a non-NULL key: the same value
    assert matched / considered == result.metrics[b.constraints[0].inner.analyzer].value.get()
    assert len(constraints) == 6


# ---- 4. compaction -------------------------------------------------------------------------------------------------
def _pylists(table):
    return {name: (_to_host(c) if c.values is None else c).to_pylist() for name, c in table.columns.items()}


@pytest.mark.parametrize("filteredRow", ["true", "null"])
@pytest.mark.parametrize("device_table", [True, False])
def test_failed_and_passed_rows_are_numpy_take(device_table, filteredRow):
    t, _, result = _e2e_run(device_table)
    null_mode = filteredRow == "null"
    res = D.VerificationResult.rowLevelResultsAsTable(result, t, filteredRow=filteredRow)
    _, (a, b) = _e2e_model(null_mode)
    data = _e2e_data()

    def false_rows(o):
        return ~o.value if o.validity is None else o.validity & ~o.value
    cases = [(res.failedRowsTable("B"), false_rows(b)), (res.passedRowsTable(), a.value & b.value),
             (res.failedRowsTable(), false_rows(a) | false_rows(b)), (res.passedRowsTable("A"), a.value)]
    for got, mask in cases:
        idx = np.flatnonzero(mask)
        assert got.nrows == len(idx) and list(got.columns) == list(t.columns)  # the data's columns, not the check columns
        assert all((c.device is not None and c.values is None) == device_table for c in got.columns.values())
        lists = _pylists(got)
        for name in t.columns:  # a string column (k2, s) and nullable ones (all) among them
            assert lists[name] == [data[name][i] for i in idx], name
    with pytest.raises(KeyError):
        res.failedRowsTable("C")


# ---- 5. shapes -----------------------------------------------------------------------------------------------------
def test_kept_dictionary_column_gives_the_decoded_columns():
    import pyarrow as pa
    rng = np.random.default_rng(5)
    n = 3001
    entries = ["w1", "w22", "", LONG_KEY, None, "x", "w1"]  # a NULL entry and a duplicate entry
    idx = rng.integers(0, len(entries), n).astype(np.int32)
    cat = pa.DictionaryArray.from_arrays(pa.array(idx, mask=rng.random(n) < 0.1), pa.array(entries, type=pa.string()))
    at = pa.table({"cat": cat, "f": pa.array(rng.integers(-2, 3, n), mask=rng.random(n) < 0.2, type=pa.int64()),
                   "u": pa.array(rng.integers(0, n, n), type=pa.int64())})
    kept, dec = Table.from_arrow(at, dictionaries="keep").to_device(0), Table.from_arrow(at).to_device(0)
    assert isinstance(kept["cat"], DictColumn)
    E = D.CheckLevel.Error
    checks = [D.Check(E, "strings").isComplete("cat").where("f > 0").hasPattern("cat", "^w").isContainedIn("cat", ["w1", "x"]),
              D.Check(E, "keys").isUnique("cat").isPrimaryKey("cat", "u").where("f > 0")]
    host = Table.from_arrow(at)
    cells = host["cat"].to_pylist()
    got = {}
    for name, t in (("kept", kept), ("decoded", dec)):
        result = D.VerificationSuite().onData(t).addChecks(checks).run()
        for mode in ("true", "null"):
            res = D.VerificationResult.rowLevelResultsAsTable(result, t, filteredRow=mode)
            assert res.skipped == []
            want_counts, outcomes = M.fold(_model_terms(0, checks[0], host) + _model_terms(1, checks[1], host), 2, n,
                                           mode == "null")
            _assert_columns(res, outcomes, ["strings", "keys"], n, mode == "null")
            assert [(m, k) for _, _, m, k in res.termCounts] == want_counts
            got[name, mode] = [_column_arrays(res.table[c], n) for c in ("strings", "keys")]
            failed = _pylists(res.failedRowsTable("strings"))
            assert failed["cat"] == [cells[i] for i in np.flatnonzero(
                ~outcomes[0].value if outcomes[0].validity is None else outcomes[0].validity & ~outcomes[0].value)]
    for mode in ("true", "null"):
        for (v1, b1), (v2, b2) in zip(got["kept", mode], got["decoded", mode]):
            assert np.array_equal(v1, v2) and (b1 is None) == (b2 is None) and (b1 is None or np.array_equal(b1, b2))


@pytest.mark.parametrize("filteredRow", ["true", "null"])
def test_chunked_table_runs_chunk_by_chunk(filteredRow):
    cut = 2051
    whole = _e2e_table().to_device(0)
    chunked = ChunkedTable([_e2e_table(slice(0, cut)).to_device(0), _e2e_table(slice(cut, None)).to_device(0)])
    checks = list(_e2e_checks())
    result = D.VerificationSuite().onData(chunked).addChecks(checks).run()
    res = D.VerificationResult.rowLevelResultsAsTable(result, chunked, filteredRow=filteredRow)
    assert isinstance(res.table, ChunkedTable) and [c.nrows for c in res.table.chunks] == [cut, N_ROWS - cut]
    # the uniqueness constraints are skipped (a group spans chunks) and left out of B's AND
    b = checks[1]
    assert [(d, k) for d, k, _ in res.skipped] == [("B", b.constraints[0]), ("B", b.constraints[1])]
    with pytest.raises(UnsupportedOnDevice):
        D.VerificationResult.rowLevelResultsAsTable(result, chunked, filteredRow=filteredRow, strict=True)
    null_mode = filteredRow == "null"
    host = _e2e_table()
    want_counts, outcomes = M.fold(_model_terms(0, checks[0], host, True) + _model_terms(1, b, host, True), 2, N_ROWS,
                                   null_mode)
    assert [(m, k) for _, _, m, k in res.termCounts] == want_counts
    # check A (no uniqueness) equals the whole table's column, chunk by chunk
    whole_res = D.VerificationResult.rowLevelResultsAsTable(D.VerificationSuite().onData(whole).addChecks(checks).run(),
                                                            whole, filteredRow=filteredRow)
    whole_a = _column_arrays(whole_res.table["A"], N_ROWS)
    for name, want in zip(["A", "B"], outcomes):
        parts = [_column_arrays(c[name], c.nrows) for c in res.table.chunks]
        vals = np.concatenate([p[0] for p in parts])
        assert np.array_equal(vals, want.value), name
        if null_mode:
            assert np.array_equal(np.concatenate([p[1] for p in parts]), want.validity), name
        assert (res.passedRows[name], res.failedRows[name], res.nullRows[name]) == \
            (want.true_rows, want.false_rows, want.null_rows)
        if name == "A":
            assert np.array_equal(vals, whole_a[0])
    failed = res.failedRowsTable("A")
    assert isinstance(failed, ChunkedTable) and failed.nrows == res.failedRows["A"]


def test_twenty_checks_take_two_native_calls():
    rng = np.random.default_rng(9)
    n = 4133
    t = Table.from_pydict({"a": [None if rng.random() < 0.2 else int(v) for v in rng.integers(0, 25, n)],
                           "f": [None if rng.random() < 0.2 else int(v) for v in rng.integers(-3, 4, n)]},
                          types={"a": "long", "f": "long"})
    E = D.CheckLevel.Error
    checks = []
    for k in range(20):
        c = D.Check(E, "check %d" % k).satisfies("a >= %d" % k, "a at least %d" % k)
        if k % 3 == 0:
            c = c.where("f > 0")
        if k % 4 == 0:
            c = c.isComplete("a")
        checks.append(c)
    host = Table.from_pydict({c: t[c].to_pylist() for c in t.columns}, types={"a": "long", "f": "long"})
    t.to_device(0)
    result = D.VerificationSuite().onData(t).addChecks(checks).run()
    ctx = engine.ctx()
    for mode in ("true", "null"):
        before = ctx.kernel_launches()["row_outcomes"]
        res = D.VerificationResult.rowLevelResultsAsTable(result, t, filteredRow=mode)
        assert ctx.kernel_launches()["row_outcomes"] - before == 2  # 16 checks, then 4
        terms = [x for k, c in enumerate(checks) for x in _model_terms(k, c, host)]
        want_counts, outcomes = M.fold(terms, 20, n, mode == "null")
        _assert_columns(res, outcomes, [c.description for c in checks], n, mode == "null")
        assert [(m, k) for _, _, m, k in res.termCounts] == want_counts


# ---- 6. many words, cheaply ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3_000_000, GRID_ROWS + 2 * TILE + 77])
def test_many_words_one_completeness_term(n):
    """One NOT_NULL term, one check: 3 000 000 rows are 184 workgroups whose per-block counts are folded with atomics;
    the second size is past what the largest grid covers in one pass, so the waves stride to a second tile. Only the
    counts and a popcount of the bitmap are compared with numpy."""
    import torch
    rng = np.random.default_rng(n & 0xFFFF)
    raw = rng.integers(0, 256, (n + 7) // 8, dtype=np.uint8)
    bitmap = np.zeros(_words(n) * 8, dtype=np.uint8)
    bitmap[:len(raw)] = raw
    want = int(np.unpackbits(raw, bitorder="little", count=n).sum())
    col = N.DqColumn()
    col.spark_type, col.flags, col.length = N.TYPE_BOOLEAN, N.COL_DEVICE, n
    values = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    validity = torch.from_numpy(bitmap).to("cuda:0")
    col.values, col.validity = values.data_ptr(), validity.data_ptr()
    term = N.DqRowTerm()
    term.kind, term.index, term.where, term.check = N.ROW_NOT_NULL, 0, -1, 0
    bufs, checks = _check_buffers(n, False, 1)
    ctx = engine.ctx()
    before = ctx.kernel_launches()["row_outcomes"]
    tc, cc = ctx.row_outcomes([col], n, [], [term], checks)
    assert ctx.kernel_launches()["row_outcomes"] - before == 1
    assert tc == [(want, n)] and cc == [(want, 0)]
    passed, out_values, _ = bufs[0]
    got = passed.cpu().numpy()
    assert int(np.unpackbits(got[:_words(n) * 8]).sum()) == want and (got[_words(n) * 8:] == 0xFF).all()
    assert int(out_values[:n].sum(dtype=torch.int64).item()) == want
    assert (out_values[(n + 15) // 16 * 16:] == 0xFF).all()
