"""The strip pipeline (K2c) on the GPU at its run, block and window edges, against the oracle, with the repair of an
abandoned pipeline switched off: the cases of tests/strip_cases.py (tests/test_strip_cases.py proves on the CPU what each of
them reaches).

Every batch is solved twice on one FIFO buffer; every pair of both solves equals ``oracle.solve`` in end cell, score, status
bits, transcript and start, and -- where the case says so -- in every cell's tie mask (bits 0-2: the strips store no M bit).
Cases with end cells are then walked from each of them (``traceback_from``) against ``oracle.traceback_from``.  All
comparisons are exact.  ``PWLIB_NO_STRIP_REPAIR=1`` throughout: a hand-over that times out is an error here
("the strip pipeline of a wide pair was abandoned"), not a slower right answer."""
import pytest

from tests import strip_cases as SC
from tests.plane_checks import bkw_of, check_masks, check_walks, okw_of

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def repair_off(monkeypatch):
    monkeypatch.setenv('PWLIB_NO_STRIP_REPAIR', '1')


class SolvedOnce:
    """The oracle, with every ``solve`` of a test item kept: both repetitions of a batch compare with one answer."""

    def __init__(self, oracle):
        self.oracle, self.kept = oracle, {}

    def solve(self, o, m, want_table=False, **kw):
        # (keyed by the arrays' identity: one SolvedOnce serves one case -- run_case makes it -- whose pairs stay alive and whose
        #  keywords are the same for every call, so they are not part of the key)
        key = (id(o), id(m), want_table)
        if key not in self.kept:
            self.kept[key] = self.oracle.solve(o, m, want_table=want_table, **kw)
        return self.kept[key]


def check_record(want, res, txs, k, label):
    from biseqt_amd import _pwlib as W
    st = int(res['status'][k])
    assert not st & W.PW_ST_BADPATH, (label, st)
    assert (int(res['opt_i'][k]), int(res['opt_j'][k])) == tuple(want['opt']), (label, res[k], want['opt'])
    if want['opt'] == (-1, -1):                       # no end cell: nothing was walked
        assert not st & (W.PW_ST_TRACED | W.PW_ST_BADPATH) and not txs[k], (label, st)
        return
    assert res['score'][k] == want['score'], (label, res['score'][k], want['score'])
    assert (bool(st & 4), bool(st & 2) and not st & 4) == (want['would_panick'], want['tb_null']), (label, st)
    if not want['would_panick'] and not want['tb_null']:
        assert txs[k] == want['transcript'], label
        assert (int(res['origin_idx'][k]), int(res['mutant_idx'][k])) == (want['origin_idx'], want['mutant_idx']), label


def run_case(oracle, c, monkeypatch):
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import BatchAligner
    if c['run_len']:
        monkeypatch.setenv('PWLIB_STRIP_RUN', str(c['run_len']))
    else:
        monkeypatch.delenv('PWLIB_STRIP_RUN', raising=False)
    kw = SC.kw_of(c)
    okw, bkw = okw_of(kw), bkw_of(kw)
    once = SolvedOnce(oracle)
    flags = W.PW_FLAG_FORCE_STRIP if c.get('forced', True) else 0
    with BatchAligner(c['pairs'], flags=flags, **bkw) as b:
        assert 'k_fill_strip' in b.kernel_name, (c['id'], b.kernel_name)
        for rep in range(2):                          # the second solve meets the granules of the first
            res = b.run()
            txs = b.transcripts(res)
            for k, (o, m) in enumerate(c['pairs']):
                label = '%s pair %d solve %d' % (c['id'], k, rep)
                if c['masks']:
                    want = check_masks(once, b, k, o, m, okw, True, label)
                else:
                    want = once.solve(o, m, **okw)
                check_record(want, res, txs, k, label)
    if c['ends']:
        o, m = c['pairs'][0]
        ends = c['ends']
        with BatchAligner([(o, m)] * len(ends), flags=flags, **bkw) as b:
            assert 'k_fill_strip' in b.kernel_name, (c['id'], b.kernel_name)
            b.solve()
            b.traceback_from(ends)
            b.sync()
            res = b.results()
            txs = b.transcripts(res)
        check_walks(oracle, o, m, okw, ends, res, txs, c['id'])


def _ids(cs):
    return [c['id'] for c in cs]


@pytest.mark.parametrize('Y', SC.GRID_Y)
def test_block_kind_grid(Y, oracle, monkeypatch):
    """Family 1, one column count per item: all seven row counts, two alignment types each, whole planes."""
    cs = [c for c in SC.family1() if len(c['pairs'][0][1]) == Y]
    assert len(cs) == 2 * len(SC.GRID_X)
    for c in cs:
        run_case(oracle, c, monkeypatch)


@pytest.mark.parametrize('run_len', (1, 2, 3, 5))
def test_run_boundaries_on_small_tables(run_len, oracle, monkeypatch):
    """Family 2: PWLIB_STRIP_RUN puts a run boundary -- another XCD, the write-through store, the cross_in polls -- between the
    strips of small tables, below and above the FAST threshold."""
    cs = [c for c in SC.family2() if c['run_len'] == run_len]
    assert len(cs) >= 8
    for c in cs:
        run_case(oracle, c, monkeypatch)


@pytest.mark.parametrize('c', SC.family3(), ids=_ids(SC.family3()))
def test_run_boundary_and_second_draw_at_the_default_placement(c, oracle, monkeypatch):
    """Family 3: tall, thin tables whose strips fill two and three runs of the default placement, and one of 1032 strips."""
    run_case(oracle, c, monkeypatch)


@pytest.mark.parametrize('c', SC.family4(), ids=_ids(SC.family4()))
def test_stale_granules_inside_one_batch(c, oracle, monkeypatch):
    """Family 4: three pairs one after another on one FIFO buffer."""
    assert len(c['pairs']) == 3
    run_case(oracle, c, monkeypatch)


def test_walker_windows(oracle, monkeypatch):
    """Family 5: I and D runs around the window's 160 steps and 4 strips, identical pairs around the ballot's 63."""
    for c in SC.family5():
        if not c['ends']:
            run_case(oracle, c, monkeypatch)


WALK_ENDS = [c for c in SC.family5() if c['ends']]


@pytest.mark.parametrize('c', WALK_ENDS, ids=_ids(WALK_ENDS))
def test_walks_from_strip_edges(c, oracle, monkeypatch):
    """Family 5: traceback_from the corners, the rows around every strip boundary and a sample of cells."""
    run_case(oracle, c, monkeypatch)


@pytest.mark.parametrize('c', SC.family6(), ids=_ids(SC.family6()))
def test_fixup_segments(c, oracle, monkeypatch):
    """Family 6: transcripts cut into one, two and three segments, on, below and above a multiple of 64 nseg ops."""
    run_case(oracle, c, monkeypatch)

