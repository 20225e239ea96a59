"""Shared pieces of the tests/test_reference_kats_*.py files: the stacks a
known-answer scenario runs on, and the two comparisons each engine case adds to
the reference's own numbers (bit-for-bit equality with the oracle, and the
whole-list Select against the per-node results)."""
import pytest

from oracle.oracle import OracleGenericStack, OracleSystemStack
from tests.helpers import assert_same_placements


class _Kind:
    """One way to build the stacks of a scenario: the oracle, the engine, or the
    engine with every full scan on the multi-CU sweep (PE_SWEEP_MIN=1; the engine
    reads its switches when a stack is created)."""

    def __init__(self, name):
        self.name = name
        self.is_oracle = name == "oracle"

    def generic(self, **kw):
        if self.is_oracle:
            return OracleGenericStack(**kw)
        from nomad_amd.stack import GenericStack
        return GenericStack(**kw)

    def system(self, **kw):
        if self.is_oracle:
            return OracleSystemStack(**kw)
        from nomad_amd.stack import SystemStack
        return SystemStack(**kw)


ORACLE = _Kind("oracle")

STACKS = [pytest.param("oracle", id="oracle"),
          pytest.param("engine", id="engine", marks=pytest.mark.gpu)]
STACKS_SWEEP = STACKS + [pytest.param("engine-sweep", id="engine-sweep", marks=pytest.mark.gpu)]


def kind_of(name, monkeypatch=None):
    if name == "engine-sweep":
        monkeypatch.setenv("PE_SWEEP_MIN", "1")
    return _Kind(name)


def mk(stack, nodes, allocs, job, metrics=False):
    stack.SetState(nodes, allocs)
    stack.SetJob(job)
    if metrics:
        stack.EnableMetrics(True)
    return stack


def _select(st, tg, options):
    """SelectRaw keeps the counters of a Select that found no node; only Select
    passes penalty and preferred nodes on, so a scenario with options must find one."""
    if options is None:
        return st.SelectRaw(tg)
    r = st.Select(tg, options)
    assert r is not None
    return r


def select_on(st, node, tg=0, options=None):
    """Select with SetNodes([node]): the chain's verdict and score parts for one node."""
    st.SetNodes([node])
    return _select(st, tg, options)


def limit_winner(finals, limit, max_skip=3):
    """LimitIterator (select.go:35-74, threshold 0, maxSkip 3) under MaxScoreIterator
    over the feasible options' final scores in visit order: up to max_skip
    non-positive options are set aside and only return once the source runs dry;
    the first of the highest returned options wins."""
    returned, aside = [], []
    for i, s in enumerate(finals):
        if len(returned) == limit:
            break
        if s <= 0 and len(aside) < max_skip:
            aside.append(i)
        else:
            returned.append(i)
    if len(returned) < limit:
        returned += aside[:limit - len(returned)]
    win = -1
    for i in returned:
        if win < 0 or finals[i] > finals[win]:
            win = i
    return win


def select_all(st, nodes, per_node, tg=0, options=None, full_scan=False):
    """The second path: one SetNodes(all) / Select. Its winner is the node the
    per-node results name (the first of the highest final scores among the options
    the limit lets through), with that node's scores. `full_scan`: the group has
    affinities or spreads, so Select lifts the limit (stack.go:152-163)."""
    limit = st.SetNodes(nodes)
    if full_scan:
        limit = 2 ** 31 - 1
    r = _select(st, tg, options)
    feasible = [(n, p) for n, p in zip(nodes, per_node) if p.row >= 0]
    if not feasible:
        assert r.row == -1
        return r
    w = limit_winner([p.final_score for _, p in feasible], limit)
    want_node, want = feasible[w]
    assert r.row == want.row, (r.row, want.row, [p.final_score for _, p in feasible])
    assert r.final_score == want.final_score and r.scores == want.scores
    return r


def both(kind, scenario):
    """Run `scenario(kind)`, which asserts the reference's values and returns the
    RankedNodes it saw; on the engine the same scenario runs on the oracle too and
    every record must agree bit for bit."""
    trace = scenario(kind)
    if not kind.is_oracle:
        assert_same_placements(trace, scenario(ORACLE))
    return trace
