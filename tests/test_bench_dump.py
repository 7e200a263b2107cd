"""bench.py --dump-outputs (host side): float arrays only, the 64 MB bound, and a sample that is the same on every run."""
import os
import subprocess
import sys

import numpy as np

import bench
from biseqt_amd import synth
from biseqt_amd.batch import RESULT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_batch(n, length=50):
    origins, mutants = synth.pair_batch(5, n, length)
    rng = synth.rng_for(6)
    res = np.zeros(n, RESULT_DTYPE)
    res['score'] = rng.integers(-5, 40, n) + 0.25
    res['opt_i'] = rng.integers(0, length, n)
    res['opt_j'] = rng.integers(0, length, n)
    res['tx_len'] = [rng.integers(0, len(o) + len(m) + 1) for o, m in zip(origins, mutants)]
    res['status'] = 1
    txs = [''.join('MSID'[c] for c in rng.integers(0, 4, t)) or None for t in res['tx_len']]
    return res, txs, origins, mutants


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_float_complete_and_repeatable(tmp_path):
    res, txs, origins, mutants = _fake_batch(3000)
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    bench.dump_outputs(a, res, txs, origins, mutants)
    bench.dump_outputs(b, res, txs, origins, mutants)
    got, again = _load(a), _load(b)
    assert sorted(got) == sorted(list(RESULT_DTYPE.names) + ['transcripts', 'transcript_pairs'])
    for name, arr in got.items():
        assert arr.dtype in (np.float32, np.float64), name
        assert np.array_equal(arr, again[name]), name
    for name in RESULT_DTYPE.names:                      # every record, exactly
        assert np.array_equal(got[name], res[name].astype(np.float64)), name
    pairs = got['transcript_pairs'].astype(np.int64)
    assert pairs.size == bench.DUMP_TX_PAIRS and np.all(np.diff(pairs) > 0)
    for row, k in enumerate(pairs):
        n = int(res['tx_len'][k])
        assert ''.join(map(chr, got['transcripts'][row, :n].astype(np.uint8))) == (txs[k] or '')
        assert not got['transcripts'][row, n:].any()


def test_dump_stays_under_64_mb(tmp_path):
    n = 1300000                                          # records alone would exceed the bound
    res, _, _, _ = _fake_batch(1)
    res = np.resize(res, n)
    origins = mutants = [np.zeros(2000, np.uint8)] * n
    txs = [None] * n
    shapes = bench.dump_outputs(str(tmp_path), res, txs, origins, mutants)
    total = sum(os.path.getsize(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path)))
    assert total <= (64 << 20) + 4096 * len(shapes)      # (npy headers)
    rec_pairs = np.load(str(tmp_path / 'record_pairs.npy'))
    assert 0 < rec_pairs.size < n and np.all(np.diff(rec_pairs) > 0)
    assert shapes['score'] == [rec_pairs.size]


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert p.returncode == 2 and '--steps' in p.stderr
