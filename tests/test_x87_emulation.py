"""
CPU test of the 80-bit add emulation used by the device solve (K3): the shared header
kbbq-py_amd/csrc/x87add.h is compiled for the host and compared with the CPU's native x87
long double arithmetic (the arithmetic np.longdouble uses on x86-64) on millions of pairs,
and against NumPy itself on a sample.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope='module')
def x87_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('native') / 'x87_check')
    src = os.path.join(ROOT, 'tests', 'native', 'x87_check.cpp')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-ffp-contract=off', '-fsanitize=undefined', '-fno-sanitize-recover=undefined', '-o', exe, src])
    return exe


@pytest.mark.skipif(np.finfo(np.longdouble).nmant != 63, reason='np.longdouble is not x87 extended here')
def test_x87_add_matches_native_long_double(x87_check):
    out = subprocess.run([x87_check, '1500000'], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith('OK')


def _key_pairs():
    """(a, b) whose 80-bit sums cover every branch of the order key: both signs, both zeros, both infinities, nan,
    neighbours in the last bit of the 64-bit significand, sums that round onto a neighbour (equal keys), and the
    smallest / largest exponents a sum of two doubles reaches (2^-1074 and 2^1024)."""
    big, tiny = 1.7976931348623157e308, 5e-324
    pairs = [(-0.10536051565782628, -648.1053605156578), (-2.1053605156578263, -3.5), (-1e-300, -1e-300),
             (1.5, 2.25), (3.0, 1e-3), (1e300, 1e300), (-7.0, 9.0), (7.0, -9.0),
             (0.0, 0.0), (-0.0, -0.0), (1.0, -1.0), (0.0, -0.0),
             (np.inf, 1.0), (np.inf, np.inf), (-np.inf, -3.0), (-np.inf, -np.inf), (np.inf, -np.inf), (-np.inf, np.inf),
             (big, big), (-big, -big), (big, 0.0), (-big, 0.0), (big, -tiny),
             (tiny, 0.0), (-tiny, 0.0), (tiny, tiny), (-tiny, -tiny), (tiny, -tiny), (2.2250738585072014e-308, -tiny)]
    for s in (1.0, -1.0):
        for base in (1.0, 648.1053605156578, 2.0 ** -40, 2.0 ** 900):
            u = base * 2.0 ** -63                                  # one unit in the last place of the 64-bit significand at 1.0 * base
            pairs += [(s * base, 0.0), (s * base, s * u), (s * base, s * 2 * u), (s * base, s * 3 * u),
                      (s * base, s * u / 2),                       # tie: rounds to even, back onto base
                      (s * base, s * u * 0.75),                    # rounds up onto base + u
                      (s * base, -s * u / 2), (s * base, -s * u / 4),   # below a power of two the spacing halves
                      (s * 2 * base, -s * u), (s * 2 * base, -s * 2 * u)]
    return np.array(pairs, dtype=np.float64)


@pytest.mark.skipif(np.finfo(np.longdouble).nmant != 63, reason='np.longdouble is not x87 extended here')
def test_x87_order_key_orders_as_long_double(x87_check):
    """The integer key the wave argmax of K3 reduces over (x87_order_key) against np.longdouble comparison, for EVERY pair of
    sums of one list: key(x) > key(y) exactly when x > y, equal keys exactly when neither is greater, nan flagged.  Real
    posteriors are all negative, so the zero and positive branches of the key run only here."""
    pairs = _key_pairs()
    out = subprocess.run([x87_check, 'key'], input=pairs.tobytes(), capture_output=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [tuple(int(x) for x in ln.split()) for ln in out.stdout.decode().split('\n') if ln]
    assert len(rows) == len(pairs)
    with np.errstate(all='ignore'):
        sums = pairs[:, 0].astype(np.longdouble) + pairs[:, 1].astype(np.longdouble)
    nan = np.isnan(sums)
    # the list really holds what it is meant to hold
    fin = sums[np.isfinite(sums) & (sums != 0)]
    assert (fin < 0).any() and (fin > 0).any() and (sums == 0).sum() >= 4 and nan.sum() == 2
    assert np.isposinf(sums).any() and np.isneginf(sums).any()
    assert np.abs(fin).min() == np.ldexp(np.longdouble(1), -1074) and np.abs(fin).max() > np.ldexp(np.longdouble(1), 1024)
    assert np.any(np.diff(np.unique(fin)) / np.abs(np.unique(fin)[1:]) <= np.ldexp(np.longdouble(1), -63))
    assert [r[2] for r in rows] == [int(x) for x in nan]
    keys = [(hi, lo) for hi, lo, _ in rows]
    n = len(rows)
    for i in range(n):
        for j in range(n):
            if nan[i] or nan[j]:
                continue                                           # the reduction never compares a flagged key
            assert (keys[i] > keys[j]) == bool(sums[i] > sums[j]), (pairs[i], pairs[j])
            assert (keys[i] == keys[j]) == (not sums[i] > sums[j] and not sums[j] > sums[i]), (pairs[i], pairs[j])
