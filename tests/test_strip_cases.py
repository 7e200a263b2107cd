"""Every case of tests/strip_cases.py reaches the edge of the strip pipeline it is named for -- proved from the shape
arithmetic restated there, from the constants read in the kernel's source and from the oracle's transcripts, so that
tests/test_gpu_strip_edges.py, which runs the same inputs on the device, is known to reach the code it is meant to
reach.  If a seed does not land, the seed changes, not the assertion.  The lane emulator then runs families 1 (a third),
5 and two pairs of 6 (see EMU_FIX) through the same StripFill / strip_walk code.  No GPU."""
import collections
import os
import re

import numpy as np
import pytest

from tests import strip_cases as SC
from tests.emu import emu

CSRC = os.path.join(os.path.dirname(__file__), '..', 'biseqt_amd', 'csrc')
_ORACLE = {}


def oracle_of(oracle, c, k=0, table=False):
    """The oracle's answer for pair k of a case (cached by the case's id; read-only)."""
    key = (c['id'], k, table)
    if key not in _ORACLE:
        o, m = c['pairs'][k]
        _ORACLE[key] = oracle.solve(o, m, L=4, want_table=table, **SC.kw_of(c))
    return _ORACLE[key]


def no_transcript(r):
    return r['opt'] == (-1, -1) or r['would_panick'] or r['tb_null']


def runs(tx):
    """Run-length form of a transcript: [(op, n), ...]."""
    return [(g.group(0)[0], len(g.group(0))) for g in re.finditer(r'(.)\1*', tx)]


def test_the_constants_are_the_kernels():
    """The copies in strip_cases.py against the source they name."""
    strip = open(os.path.join(CSRC, 'pw_strip.h')).read()
    api = open(os.path.join(CSRC, 'pwlib_api.cpp')).read()
    trace = open(os.path.join(CSRC, 'pw_trace.hip')).read()
    kern = open(os.path.join(CSRC, 'pw_strip.hip')).read()
    why = 're-derive family %s of tests/strip_cases.py'
    assert 'constexpr int kStripBlock = %d;' % SC.STRIP_BLOCK in strip, why % '1 (GRID_Y: the block of 32)'
    assert '#define PW_STRIP_SUB %d ' % SC.STRIP_SUB in strip, why % '1 (GRID_Y: the sub-chunk of 16)'
    assert strip.count('a.Y > %d' % SC.FAST_Y) == 2, why % '1 and 2 (the FAST threshold)'
    assert 'const int q_end = a.Y > 128 ? (q_last_cell < a.nkq - 3 ? q_last_cell : a.nkq - 3) : 0;' in strip, why % '1 (q_end)'
    assert 'const int q_last_cell = a.Y >= kStripBlock ? (a.Y - kStripBlock) / kStripBlock + 1 : 0;' in strip, why % '1 (q_last_cell)'
    assert 'const bool whole = a.Y > 128 && 64 * w + 63 <= a.X;' in strip, why % '1 (whole)'
    assert 'const bool starting = k0 < 64 && whole;' in strip and 'const bool ending = k0 >= 64 && whole;' in strip, why % '1 (block kinds)'
    assert 'if (q >= 2 && q < q_end) {' in strip, why % '1 (steady blocks)'
    assert '#define PW_WALK_STRIPS %d\n' % SC.WALK_STRIPS in strip, why % '5 (the D runs: strips per window)'
    assert 'constexpr int kWalkGroups = %d;' % SC.WALK_GROUPS in strip, why % '5 (the I runs: 32-step groups per strip)'
    assert 'run0 < 63' in strip, why % '5 (the identical pairs: the ballot\'s sentinel)'
    assert 'PW_FN uint32_t tag_of(int y) const { return (a.epoch << 8) | ((uint32_t)y & 0xffu); }' in strip, why % '1 (Y 255 .. 257) and 4'
    assert 'PW_FN int strip_fifo_pitch(int Y) { return (Y + 1 + 32 + 63) / 64 * 64; }' in strip, why % '4'
    assert 'static inline int strip_count(int X) { return (X + 1 + 63) / 64; }' in strip, why % '1 to 3'
    assert 'static inline int strip_nkq(int Y) { return (Y + 64 + kStripBlock - 1) / kStripBlock; }' in strip, why % '1'
    assert 'longest / %d' % SC.FIX_OPS in api and 'std::min<int64_t>(%d, std::max<int64_t>(1, longest / ' % SC.FIX_MAX in api, why % '6'
    assert 'd.tx_cap = p.origin_len + p.mutant_len + 1;' in api, why % '6 (tx_cap)'
    assert 'const int seglen = ((r.tx_len + nseg - 1) / nseg + 63) & ~63;' in trace, why % '6 (seglen)'
    assert '"PWLIB_STRIP_WAVES", %d' % SC.WORKERS in api, why % '3 (the second draw)'
    assert 'env_int("PWLIB_STRIP_RUN", std::max(1, workers / a.nq))' in api, why % '2 and 3 (the run length)'
    assert 'f.run(w, i == 0, i == a.run_len - 1);' in kern, why % '2 and 3 (first and last of a run)'
    # the arithmetic itself, at the shapes the comments of pw_strip.h give
    assert (SC.strip_count(0), SC.strip_count(63), SC.strip_count(64)) == (1, 1, 2)
    assert (SC.strip_nkq(0), SC.strip_nkq(1), SC.strip_nkq(128), SC.strip_nkq(129)) == (2, 3, 6, 7)
    assert (SC.strip_fifo_pitch(0), SC.strip_fifo_pitch(31), SC.strip_fifo_pitch(32)) == (64, 64, 128)


def test_case_ids_are_unique_and_the_grid_is_whole():
    cs = SC.cases()
    assert len({c['id'] for c in cs}) == len(cs)
    f1 = SC.family1()
    assert {(len(o), len(m)) for c in f1 for o, m in c['pairs']} == {(X, Y) for X in SC.GRID_X for Y in SC.GRID_Y}
    assert 200 <= len(f1) <= 400 and all(c['masks'] for c in f1)
    assert {X % 64 for X in SC.GRID_X} >= {0, 1, 63} and {SC.strip_count(X) for X in SC.GRID_X} >= {1, 11}
    for c in cs:
        sc = c['score']
        assert (sc is SC.MAT or sc in SC.SCORES) and (SC.MAT[1] if sc is SC.MAT else sc[2]) <= 0, c['id']      # (no M bit: go <= 0)


def test_every_block_kind_meets_every_alignment_type():
    met = collections.defaultdict(set)
    last_whole = set()
    for c in SC.family1():
        (o, m), = c['pairs']
        X, Y = len(o), len(m)
        met[c['alntype']] |= SC.block_kinds(X, Y)
        if Y > SC.FAST_Y:
            last_whole.add(SC.whole(X, Y, SC.strip_count(X) - 1))
    assert sorted(met) == list(range(7))
    for t, kinds in met.items():
        assert kinds == set(SC.KINDS), (t, sorted(set(SC.KINDS) - kinds))
    assert last_whole == {True, False}
    # q_end is the smaller of q_last_cell = Y / 32 and nkq - 3 = (Y - 1) / 32: the latter, which grows at Y = 161, 193, ...
    assert all(SC.q_end(Y) == (Y - 1) // 32 <= SC.q_last_cell(Y) for Y in range(SC.FAST_Y + 1, 400))
    assert [SC.q_end(Y) for Y in (128, 129, 159, 160, 161, 200, 300)] == [0, 4, 4, 4, 5, 6, 9]


def test_run_boundaries_are_crossed_below_and_above_the_fast_threshold():
    by_run = collections.defaultdict(set)
    for c in SC.family2():
        (o, m), = c['pairs']
        assert c['masks'] and SC.runs_of(len(o), c['run_len']) >= 2, c['id']
        assert 3 <= SC.strip_count(len(o)) <= 11 or (c['run_len'] == 5 and SC.strip_count(len(o)) == 41), c['id']
        by_run[c['run_len']].add(len(m) > SC.FAST_Y)
    assert sorted(by_run) == [1, 2, 3, 5]
    assert all(v == {True, False} for v in by_run.values()), dict(by_run)


def test_the_tall_tables_cross_runs_and_draw_twice():
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import plan_only
    f3 = SC.family3()
    assert max(SC.runs_of(len(c['pairs'][0][0]), None) for c in f3) >= 3
    assert {SC.runs_of(len(c['pairs'][0][0]), None) for c in f3} >= {2, 3}
    draw2 = [c for c in f3 if SC.strip_count(len(c['pairs'][0][0])) > SC.WORKERS]
    assert draw2 and all(SC.strip_count(len(c['pairs'][0][0])) - SC.WORKERS == 8 for c in draw2)
    assert {c['alntype'] for c in f3} == {0, 1, 4, 6}
    assert {len(c['pairs'][0][1]) for c in f3} >= {1, 17, 129, 300}
    for c in f3:
        (o, m), = c['pairs']
        assert c['masks'] == ((len(o) + 1) * (len(m) + 1) <= SC.MASK_CELLS), c['id']
        kw = SC.kw_of(c)
        plan = plan_only([(len(o), len(m))], alnmode=0, alntype=kw['alntype'], match_score=kw['match'], mismatch_score=kw['mismatch'],
                         go_score=kw['go'], ge_score=kw['ge'], flags=W.PW_FLAG_FORCE_STRIP if c['forced'] else 0)
        assert 'k_fill_strip' in plan['kernel'] and plan['strips'] == 1, (c['id'], plan)


def test_the_walker_cases_hold_single_runs(oracle):
    for c in SC.family5():
        r = oracle_of(oracle, c)
        assert not no_transcript(r), c['id']
        (o, m), = c['pairs']
        if 'gap' in c:
            g, f = c['gap'], c['flank']
            assert runs(r['transcript']) == [('M', f), (c['op'], g), ('M', f)], (c['id'], runs(r['transcript']))
            # an I run stays in one strip; a D run of g rows crosses g / 64 strip boundaries at least
            if c['op'] == 'I':
                assert f % 64 != 0 and g >= 32 * SC.WALK_GROUPS - 1
            else:
                assert (f + g) // 64 - f // 64 >= min(g // 64, SC.WALK_STRIPS - 1)
        else:
            assert runs(r['transcript']) == [('M', len(o))] and np.array_equal(o, m), c['id']
    big = {c['id']: oracle_of(oracle, c) for c in SC.family5() if c.get('gap') == 300}
    assert sorted(big) == ['walk-D300', 'walk-I300']
    assert big['walk-I300']['transcript'] == 'M' * 400 + 'I' * 300 + 'M' * 400 and big['walk-I300']['score'] == 195
    assert big['walk-D300']['transcript'] == 'M' * 400 + 'D' * 300 + 'M' * 400 and big['walk-D300']['score'] == 195
    assert (400 + 300) // 64 - 400 // 64 >= SC.WALK_STRIPS                   # the D run: five strips, one more than a window
    with_ends = [c for c in SC.family5() if c['ends']]
    assert len(with_ends) == 2
    for c in with_ends:
        (o, m), = c['pairs']
        X, Y = len(o), len(m)
        e = set(c['ends'])
        assert {(0, 0), (0, Y), (X, 0), (X, Y)} <= e and len(c['ends']) >= 200 + 4 + 12 * (X // 64)
        assert all((64 * k + d, y) in e for k in range(1, X // 64 + 1) for d in (-1, 0, 1) for y in (0, 1, Y - 1, Y) if 64 * k + d <= X)
        assert all(0 <= x <= X and 0 <= y <= Y for x, y in e)


def test_the_fixup_cases_cut_where_they_say(oracle):
    nsegs, on_multiple = set(), set()
    for c in SC.family6():
        for k in range(len(c['pairs'])):
            r = oracle_of(oracle, c, k)
            assert not no_transcript(r), (c['id'], k)
            nseg, seglen = SC.fixup_segments(c['pairs'], len(r['transcript']))
            if k == 0:
                nsegs.add(nseg)
                if len(r['transcript']) % (64 * nseg) == 0:
                    on_multiple.add(nseg)
    assert nsegs == {1, 2, 3} and on_multiple >= {2, 3}, (nsegs, on_multiple)
    by_id = {c['id']: c for c in SC.family6()}
    for n, want in zip(SC.FIX_SIZES, (1, 2, 2, 2, 3, 3)):
        c = by_id['fix-identical-%d-global' % n]
        assert SC.fixup_segments(c['pairs'], n)[0] == want and len(oracle_of(oracle, c)['transcript']) == n
    # the short pair beside a long one: every segment but its first is empty
    c = by_id['fix-beside-a-short-pair']
    short = oracle_of(oracle, c, 1)
    nseg, seglen = SC.fixup_segments(c['pairs'], len(short['transcript']))
    assert nseg == 2 and 0 < len(short['transcript']) <= seglen
    # indels in the 128 ops in front of the second segment, and a start away from the origin
    c = by_id['fix-indels-before-a-cut']
    r = oracle_of(oracle, c)
    nseg, seglen = SC.fixup_segments(c['pairs'], len(r['transcript']))
    before = r['transcript'][seglen - 128:seglen]
    assert nseg == 2 and seglen < len(r['transcript']) and 'I' in before and 'D' in before, (nseg, seglen, runs(before))
    assert r['origin_idx'] > 64 and r['mutant_idx'] > 64 and r['origin_idx'] != r['mutant_idx']


def test_few_cases_have_no_transcript_to_compare(oracle):
    """The cap that keeps the GPU test honest: a case whose oracle answer has no transcript (opt == (-1, -1), would_panick or
    tb_null) is compared on opt, score and status only.  At most 10 % of the list and 25 % of any alignment type; none in
    families 5 and 6."""
    tot, no = collections.Counter(), collections.Counter()
    for c in SC.cases():
        for k in range(len(c['pairs'])):
            bad = no_transcript(oracle_of(oracle, c, k))
            tot[c['alntype']] += 1
            no[c['alntype']] += bad
            assert not (bad and c['family'] in (5, 6)), c['id']
    share = {t: no[t] / tot[t] for t in tot}
    overall = sum(no.values()) / sum(tot.values())
    print('cases without a transcript: %.1f %% overall; per type %s' % (100 * overall, {t: '%d of %d' % (no[t], tot[t]) for t in sorted(tot)}))
    assert sorted(tot) == list(range(7))
    assert overall <= 0.10, overall
    assert max(share.values()) <= 0.25, share


# ---- the lane emulator on the same inputs --------------------------------------------------------------------
def emu_check(oracle, c, masks, only=None):
    kw = SC.kw_of(c)
    for k, (o, m) in enumerate(c['pairs']):
        if only is not None and k != only:
            continue
        want = oracle_of(oracle, c, k, table=masks)
        ekw = dict(kw)
        ekw.pop('mode')
        got = emu.solve_strip(o, m, want_masks=masks, **ekw)
        label = (c['id'], k)
        assert got['init_rc'] == 0 and got['opt'] == want['opt'], label
        if want['opt'] == (-1, -1):
            continue
        assert got['score'] == want['score'] and not got['badpath'], label
        assert (got['would_panick'], got['tb_null']) == (want['would_panick'], want['tb_null']), label
        if not no_transcript(want):
            assert got['transcript'] == want['transcript'], label
            assert (got['origin_idx'], got['mutant_idx']) == (want['origin_idx'], want['mutant_idx']), label
        if masks:
            bad = np.nonzero((got['mask'] & 7) != (want['mask'] & 7))[0]
            assert bad.size == 0, (label, '%d of %d cells differ' % (bad.size, got['mask'].size), bad[:8].tolist())


@pytest.mark.parametrize('part', range(7))
def test_emulated_grid(part, oracle):
    """A third of family 1 (7 of every 21 cases in list order: every X, every type, 14 cases per part) with whole planes."""
    for c in SC.family1()[part::21]:
        emu_check(oracle, c, True)


def test_emulated_walker_cases(oracle):
    for c in SC.family5():
        emu_check(oracle, c, True)


# Family 6 is thinned to two items here, for two reasons.  The emulator's fix-up is the serial one (trace_fixup_serial) and it
# solves one pair at a time: nseg, seglen and the cut -- what family 6 is about -- do not exist in it, so these cases show it only
# the fill and the walker on a square table of 2047 .. 3073 rows, the same lane program at every one of the 26.  And it takes
# 4 us per cell, 17 s for a 2047-row table and 31 s for a 3072-row one: the family would take ten minutes, where the file is to
# stay near one.  So: one pair of the smallest size (a walk of 2047 ops with indels through 32 strips) and the short pair that
# sits beside a long one.  The segment cut is tested on the device only (test_gpu_strip_edges.py::test_fixup_segments).
EMU_FIX = [('fix-mutated-2047-local', 0), ('fix-beside-a-short-pair', 1)]


@pytest.mark.parametrize('cid,k', EMU_FIX, ids=[i for i, _ in EMU_FIX])
def test_emulated_fixup_cases(cid, k, oracle):
    c, = [c for c in SC.family6() if c['id'] == cid]
    emu_check(oracle, c, False, only=k)
