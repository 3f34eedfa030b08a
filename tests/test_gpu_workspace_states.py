"""GPU test: every call that draws its scratch from a workspace lane (csrc/corb_workspace.h) gives the same bits whatever the lane held before it.

A lane's arena is rewound, not cleared, between calls, and its page-locked staging is reused the same way, so a call finds the leftovers of the call before it at the
addresses it is about to use; the first call of a size copies directly where later ones copy through the staging.  The rule that makes this harmless -- a call reads
nothing from the arena or the staging that it has not written itself -- is kept by hand, one allocation at a time, and a forgotten preset passes every other test,
because memory fresh from the runtime happens to be zero.  Here every entry of tests/workspace_cases.py runs in these states, in this order:
  1. fresh      corb_release_scratch first: a new arena, no staging yet, direct copies
  2. warm       again: the staging now has the size state 1 asked for, the copies are staged
  3. pattern A  both lanes filled with 0x00000001 before every call on a lane: as an integer 1 -- a plausible count, flag or index; as a float a denormal
  4. pattern B  filled with 0x3F800000: 1.0 as a float, ~0.0078 as a double -- an accumulator, weight or score that starts from it goes visibly wrong
  5. after a bigger call of the same entry point (where the entry names one): stale tails of the host's thread-local vectors and of the arena beyond the small case
and the test asserts
  (a) the outputs of all states are equal byte for byte, array by array, NaN by bit pattern -- no tolerance anywhere;
  (b) the existing test's own assertions (its reference, its bar) pass on the outputs of the pattern states, and of the others;
  (c) the fill was used: after every call of states 3 and 4 the lane is still the one filled chunk (the call took nothing outside the filled memory), and the first
      megabyte of the entry's lane no longer holds the pattern everywhere (the call wrote into the filled chunk) -- for every symbol the entry names, STAGING_ONLY's
      two apart.
Pattern B lives in a test function of its own behind the first one: an index read from unwritten memory would still be small under pattern A and is wild under B.
So an entry's pattern-B case fails at once, without a call on the GPU, unless that entry has passed states 1 to 3 in this process; where the first function is not
part of the run at all (pattern B in a command of its own), the case goes through fresh and pattern A itself before it fills with B.
Lane 0's entries come before lane 1's, so a fault in one family does not spread over the file.  Each case takes a few seconds at most."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workspace_cases as W  # noqa: E402

pytestmark = pytest.mark.gpu

# Outputs of which the header defines only a part (entries past a returned count) are compared up to that count only.  This table is the only exemption:
# {entry name: {output key: the output key of its count}}.  It is empty: the wrappers of corb-slam_amd/__init__.py cut every such array (matches past n_matches,
# pairs past n_pairs, events past n_events, chi2 past iters_done ...) at its count before they return it, so no output of the registry carries an undefined tail.
PARTIAL_OUTPUTS = {}

# Assertion (c) holds for every symbol of an entry, not only for the entry as a whole: each of them has written into the first megabyte of the filled chunk.  The
# only symbols let off are the ones named here, which allocate nothing from the arena: they move a few scalars through the page-locked staging straight into (out
# of) the graph's own rows (corb_covis.cpp: pool.h2d / pool.d2h on g->T).
STAGING_ONLY = frozenset(("corb_covis_set_tree", "corb_covis_get_tree"))

ENTRIES = sorted(W.ENTRIES, key=lambda e: e.lane)               # (stable: lane 0 in the registry's order, then lane 1)
FIRST = "test_fresh_warm_and_pattern_a_give_the_same_bytes"
_fresh = {}                                                        # entry name -> the outputs of state 1, the baseline of pattern B: set when states 1 to 3 have passed
_started = set()                                                   # the entries whose states 1 to 3 have begun in this process


def _defined(entry, out):
    part = PARTIAL_OUTPUTS.get(entry.name, {})
    return {k: (v[: int(out[part[k]])] if k in part else v) for k, v in out.items()}


def _same(entry, state, base, out):
    diff = W.same_bytes(_defined(entry, base), _defined(entry, out))
    stopped = ["; the '%s' run stopped at: %r" % (s, e) for s, e in ((state, out.error), ("fresh", base.error)) if e is not None]
    assert diff is None, "%s: state '%s' differs from 'fresh': %s%s" % (entry.name, state, diff, "".join(stopped))


def _fill_was_used(corb, entry, word):
    rec = entry.last
    assert not rec.problems, rec.problems[:3]
    assert rec.filled, "%s: no call of the entry takes a lane" % entry.name
    for lane in (0, 1):
        assert corb.scratch_report(lane)[:2] == (rec.filled[lane], 1)
    assert entry.lane in rec.written, "%s: no call wrote into the first MB of lane %d's filled chunk (wrote into: %s)" % (entry.name, entry.lane, sorted(rec.written))
    quiet = set(entry.symbols) - set().union(*rec.written.values())
    print("%s, word %08x: wrote into the first MB: %s; did not: %s" % (entry.name, word, {l: sorted(v) for l, v in rec.written.items()}, sorted(quiet)))
    assert quiet <= STAGING_ONLY, "%s: no call of %s wrote into the first MB of the filled chunk" % (entry.name, sorted(quiet - STAGING_ONLY))


def _pattern_run(corb, synth, pyorc, entry, word):
    out = entry.run(corb, synth, pyorc, word=word)
    _fill_was_used(corb, entry, word)
    return out


@pytest.mark.parametrize("entry", ENTRIES, ids=[e.name for e in ENTRIES])
def test_fresh_warm_and_pattern_a_give_the_same_bytes(corb, synth, pyorc, entry):
    _started.add(entry.name)
    corb.release_scratch(0)
    for lane in (0, 1):
        assert corb.scratch_report(lane) == (0, 0, 0)
    runs = [("fresh", entry.run(corb, synth, pyorc))]
    called = entry.last.called
    assert set(entry.symbols) <= called, "%s names %s, which its body never calls" % (entry.name, sorted(set(entry.symbols) - called))
    runs.append(("warm", entry.run(corb, synth, pyorc)))
    runs.append(("pattern A", _pattern_run(corb, synth, pyorc, entry, W.PATTERN_A)))
    assert len(runs[0][1]) > 0
    for state, out in runs[1:]:
        _same(entry, state, runs[0][1], out)                       # (a)
    for state, out in runs[::-1]:                                  # (b): pattern A's outputs against the entry point's own reference, then the others'
        entry.check(out)
    if entry.bigger is not None:
        entry.check(entry.run(corb, synth, pyorc, body=entry.bigger))
        after = entry.run(corb, synth, pyorc)
        _same(entry, "after a bigger call", runs[0][1], after)
        entry.check(after)
    _fresh[entry.name] = runs[0][1]


@pytest.mark.parametrize("entry", ENTRIES, ids=[e.name for e in ENTRIES])
def test_pattern_b_gives_the_same_bytes(request, corb, synth, pyorc, entry):
    base = _fresh.get(entry.name)
    if base is None:
        in_this_run = any(i.name == "%s[%s]" % (FIRST, entry.name) for i in request.session.items)
        assert not in_this_run and entry.name not in _started, "%s has not passed states 1 to 3 in this run: pattern B is not tried on it" % entry.name
        corb.release_scratch(0)
        base = entry.run(corb, synth, pyorc)
        entry.check(base)
        a = _pattern_run(corb, synth, pyorc, entry, W.PATTERN_A)
        _same(entry, "pattern A", base, a)
        entry.check(a)
    out = _pattern_run(corb, synth, pyorc, entry, W.PATTERN_B)
    _same(entry, "pattern B", base, out)
    entry.check(out)


def test_the_aids_fill_report_and_read(corb):
    """corb_scratch_fill / _report / _read themselves: one chunk of the size asked for (or of what the arena had, if more), every word the pattern, a range check"""
    corb.release_scratch(0)
    import numpy as np
    for lane in (0, 1):
        assert corb.scratch_fill(lane, 0xDEADBEEF, 3 << 20) == 3 << 20
        cap, chunks, staging = corb.scratch_report(lane)
        assert (cap, chunks, staging) == (3 << 20, 1, 0)
        assert (corb.scratch_read(lane, (3 << 20) - 4096, 4096).view(np.uint32) == 0xDEADBEEF).all() and (corb.scratch_read(lane, 0, 1 << 20).view(np.uint32) == 0xDEADBEEF).all()
        assert corb.scratch_fill(lane, 7, 1 << 20) == 3 << 20                                      # never smaller than it was
        assert (corb.scratch_read(lane, 1 << 20, 64).view(np.uint32) == 7).all()
        with pytest.raises(corb.CorbError):
            corb.scratch_read(lane, (3 << 20) - 8, 16)
    with pytest.raises(corb.CorbError):
        corb.scratch_fill(2, 0, 0)
    corb.release_scratch(0)
    with pytest.raises(corb.CorbError):
        corb.scratch_read(0, 0, 4)                                                                  # no chunk at all
