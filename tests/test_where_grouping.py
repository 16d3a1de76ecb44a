"""`where` on the grouping analyzers and ApproxQuantile, the host side: the analyzers as values (equality, hash, repr,
the unfiltered ones exactly as before), the runner's sharing key, and `.where(...)` on the checks built on them.
No GPU needed."""
import pytest

import deequ_amd as D
from deequ_amd import runners
from deequ_amd.checks import Check, CheckLevel, CheckWithLastConstraintFilterable

W = "status = 'shipped'"


def _pairs():
    """(unfiltered, filtered, the unfiltered repr pinned literally) of the seven analyzers."""
    return [
        (D.Uniqueness(["a", "b"]), D.Uniqueness(["a", "b"], W), "Uniqueness(List(a, b))"),
        (D.Distinctness(["a"]), D.Distinctness(["a"], where=W), "Distinctness(List(a))"),
        (D.UniqueValueRatio(["a"]), D.UniqueValueRatio(["a"], W), "UniqueValueRatio(List(a))"),
        (D.CountDistinct(["a", "b"]), D.CountDistinct(["a", "b"], W), "CountDistinct(List(a, b))"),
        (D.Entropy("a"), D.Entropy("a", W), "Entropy(a)"),
        (D.MutualInformation(["a", "b"]), D.MutualInformation(["a", "b"], W), "MutualInformation(List(a, b))"),
        (D.ApproxQuantile("x", 0.5), D.ApproxQuantile("x", 0.5, 0.01, W), "ApproxQuantile(x,0.5,0.01)"),
    ]


def test_unfiltered_analyzers_are_the_values_they_were():
    for plain, _, text in _pairs():
        assert repr(plain) == text
        assert plain.where is None
        again = type(plain)(*[getattr(plain, f) for f in plain._fields])
        assert plain == again and hash(plain) == hash(again)
        # the key is the class name and the case-class fields, nothing about a filter
        assert plain._key() == (type(plain).__name__,) + tuple(
            tuple(v) if isinstance(v, list) else v for v in (getattr(plain, f) for f in plain._fields))
        explicit = type(plain)(*[getattr(plain, f) for f in plain._fields], where=None)
        assert explicit == plain and hash(explicit) == hash(plain) and repr(explicit) == text


def test_filtered_analyzers_differ_by_their_filter_and_print_it():
    for plain, filtered, text in _pairs():
        assert filtered.where == W
        assert filtered != plain and plain != filtered
        assert repr(filtered) == text[:-1] + ",Some(%s))" % W
        same = type(plain)(*[getattr(plain, f) for f in plain._fields], where=W)
        other = type(plain)(*[getattr(plain, f) for f in plain._fields], where="status = 'open'")
        assert same == filtered and hash(same) == hash(filtered)
        assert other != filtered
        assert len({plain, filtered, same, other}) == 3
        # a state provider names a state by the repr: the filtered and the unfiltered state are different files
        assert D.HdfsStateProvider.toIdentifier(plain) != D.HdfsStateProvider.toIdentifier(filtered)


def test_metric_name_instance_and_entity_do_not_change():
    err = ValueError("x")
    for plain, filtered, _ in _pairs():
        a, b = plain.toFailureMetric(err), filtered.toFailureMetric(err)
        assert (a.name, a.instance, a.entity) == (b.name, b.instance, b.entity)


def test_the_runner_shares_a_table_per_columns_and_filter():
    key = runners._grouping_key
    assert key(D.Uniqueness(["b", "a"], W)) == key(D.Distinctness(["a", "b"], W)) == (("a", "b"), W)
    assert key(D.Entropy("a", W)) == key(D.CountDistinct(["a"], W))
    assert key(D.Uniqueness(["a"])) == (("a",), None)
    assert key(D.Uniqueness(["a"], W)) != key(D.Uniqueness(["a"]))
    assert key(D.Uniqueness(["a"], W)) != key(D.Uniqueness(["a"], "x > 1"))


CHECKS = [
    (lambda c: c.isUnique("id"), D.Uniqueness),
    (lambda c: c.isPrimaryKey("id", "part"), D.Uniqueness),
    (lambda c: c.hasUniqueness(["id", "part"], lambda v: v == 1.0), D.Uniqueness),
    (lambda c: c.hasDistinctness(["id"], lambda v: v > 0.5), D.Distinctness),
    (lambda c: c.hasUniqueValueRatio(["id"], lambda v: v > 0.5), D.UniqueValueRatio),
    (lambda c: c.hasEntropy("id", lambda v: v > 0.0), D.Entropy),
    (lambda c: c.hasMutualInformation("id", "part", lambda v: v >= 0.0), D.MutualInformation),
    (lambda c: c.hasApproxQuantile("x", 0.5, lambda v: v > 0.0), D.ApproxQuantile),
]


@pytest.mark.parametrize("k", range(len(CHECKS)))
def test_every_listed_check_takes_where(k):
    build, cls = CHECKS[k]
    base = Check(CheckLevel.Error, "c").isComplete("other")
    plain = build(base)
    assert isinstance(plain, CheckWithLastConstraintFilterable) and isinstance(plain, Check)
    (a0, a1) = plain.requiredAnalyzers()
    assert isinstance(a1, cls) and a1.where is None
    filtered = plain.where(W)
    assert isinstance(filtered, Check) and len(filtered.constraints) == len(plain.constraints) == 2
    (b0, b1) = filtered.requiredAnalyzers()
    assert b0 == a0 and b0.where is None  # only the last constraint is rebuilt
    assert type(b1) is cls and b1.where == W and b1 != a1
    assert [getattr(b1, f) for f in b1._fields] == [getattr(a1, f) for f in a1._fields]
    assert W in repr(filtered.constraints[-1])
