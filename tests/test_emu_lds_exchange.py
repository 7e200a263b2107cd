"""The two lane-crossing offers of the packed kernels behind their entry points (pw_wave.h, offer_up / offer_left), on the CPU.

Host forms.  A small program of this test's own, compiled from the text below, includes pw_wave.h with a 64-lane lockstep
platform of two passes (every lane hands on, then every lane takes) and holds, lane by lane,
  * the host form -- today's DPP move into the carried register and the alignbit;
  * the expression it replaces, written out on plain integers: (lane below's own.hi, own.lo) for the up offer, lane 0 keeping
    the seed; (own.hi, next lane's own.lo) for the left offer, lane 63 keeping the seed;
  * a model of what the device form stores and reads (WaveFill16, XLDS): two arrays of 64 + 1 dwords as halfwords, own.lo to
    the high half of word `lane`, own.hi to the low half of word `lane + 1`, the up offer taken as word `lane`, the left
    offer as word `lane + 1`, U[0].lo and L[64].hi seeded once -- every lane hands on before any lane takes, as the
    wavefront's in-order LDS operations do
against each other: all 2^16 values of one half times six values of the other half, in either half, with lane-dependent
values so that a wrong neighbour shows, at lane 0, an inner lane, lane 50 (config 2's last active lane), lane 63 and every
other lane; twice in a row, so that the carried register of the first exchange feeds the second.

The lane program.  Every form of WaveFill16 takes its offers through the same two functions, so the pair-key cases of
tests/pair_keys_cases.py run once more through them on the lane emulator (tests/emu, untouched): records, transcripts and
whole planes equal to the oracle's, as tests/test_emu_pair_keys.py holds them.
"""
import ctypes
import os
import subprocess

import pytest

from tests import pair_keys_cases as PC
from tests import test_emu_pair_keys as PK
from tests.test_emu_pair_keys import form          # noqa: F401  (the fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'biseqt_amd', 'csrc')

PROGRAM = r'''
#include <stdint.h>
#include <string.h>
#define PW_FN inline
#include "pw_wave.h"

namespace {
struct TwoPass {                    // pass 0: every lane hands its value on; pass 1: every lane reads its neighbour's
  static int cur, pass;
  static int32_t vals[64];
  static int32_t move(int32_t v, int src, int32_t old) {
    if (pass == 0) { vals[cur] = v; return 0; }
    return (src >= 0 && src < 64) ? vals[src] : old;
  }
  static int32_t shr1(int32_t v, int32_t old) { return move(v, cur - 1, old); }
  static int32_t shl1(int32_t v, int32_t old) { return move(v, cur + 1, old); }
};
int TwoPass::cur = 0, TwoPass::pass = 0;
int32_t TwoPass::vals[64];

template <bool UP> uint32_t hand_on_and_take(const uint32_t* own, uint32_t* carried, uint32_t* taken) {
  for (TwoPass::pass = 0; TwoPass::pass < 2; TwoPass::pass++)
    for (int l = 0; l < 64; l++) {
      TwoPass::cur = l;
      uint32_t c = carried[l];
      if (UP) pw::offer_up<TwoPass, false, false>(0u, c, own[l]); else pw::offer_left<TwoPass, false, false>(0u, c, own[l]);
      if (TwoPass::pass == 1) carried[l] = c;
    }
  for (int l = 0; l < 64; l++) {
    TwoPass::cur = l;
    taken[l] = UP ? pw::offer_up<TwoPass, false, true>(0u, carried[l], own[l]) : pw::offer_left<TwoPass, false, true>(0u, carried[l], own[l]);
  }
  return 0;
}
}  // namespace

// One exchange of each kind repeated `rounds` times over lane-dependent values built from (h, c, swap); returns the number of
// lanes and rounds at which the host form, the plain expression and the model of the device's arrays disagree.
extern "C" unsigned lds_exchange_check(unsigned c, int swap, unsigned seed, int rounds, unsigned* first_bad) {
  unsigned bad = 0;
  static uint16_t U[2 * pw::kOfferWords], L[2 * pw::kOfferWords];
  for (unsigned h = 0; h < 65536u; h++) {
    uint32_t own[64], carU[64], carL[64], takeU[64], takeL[64], prevU[64], prevL[64];
    memset(U, 0xa5, sizeof U); memset(L, 0xa5, sizeof L);
    for (int l = 0; l < 64; l++) { carU[l] = carL[l] = seed; prevU[l] = prevL[l] = seed; }
    U[0] = (uint16_t)(seed >> 16);                                   // U[0].lo: lane 0's carried register, its high half
    L[2 * 64 + 1] = (uint16_t)seed;                                  // L[64].hi: lane 63's carried register, its low half
    for (int r = 0; r < rounds; r++) {
      for (int l = 0; l < 64; l++) {
        const uint32_t a = (h + 0x0101u * (unsigned)l + 0x3u * (unsigned)r) & 0xffffu, b = (c + 0x1003u * (unsigned)l + (unsigned)r) & 0xffffu;
        own[l] = swap ? (b | (a << 16)) : (a | (b << 16));
      }
      hand_on_and_take<true>(own, carU, takeU);
      hand_on_and_take<false>(own, carL, takeL);
      for (int l = 0; l < 64; l++) {                                 // the device's stores: every lane, then every read
        U[2 * l + 1] = (uint16_t)own[l]; U[2 * (l + 1)] = (uint16_t)(own[l] >> 16);
        L[2 * l + 1] = (uint16_t)own[l]; L[2 * (l + 1)] = (uint16_t)(own[l] >> 16);
      }
      for (int l = 0; l < 64; l++) {
        const uint32_t below = l > 0 ? own[l - 1] : prevU[0], next = l < 63 ? own[l + 1] : prevL[63];
        const uint32_t wantU = (below >> 16) | (own[l] << 16), wantL = (own[l] >> 16) | (next << 16);
        const uint32_t devU = (uint32_t)U[2 * l] | ((uint32_t)U[2 * l + 1] << 16);
        const uint32_t devL = (uint32_t)L[2 * (l + 1)] | ((uint32_t)L[2 * (l + 1) + 1] << 16);
        if (takeU[l] != wantU || takeL[l] != wantL || devU != wantU || devL != wantL) {
          if (!bad && first_bad) { first_bad[0] = h; first_bad[1] = (unsigned)l; first_bad[2] = (unsigned)r; first_bad[3] = takeU[l]; first_bad[4] = wantU; first_bad[5] = devU; first_bad[6] = takeL[l]; first_bad[7] = wantL; first_bad[8] = devL; }
          bad++;
        }
      }
      // (the edge lanes keep what they held: lane 0's carried up offer and lane 63's carried left offer stay the seed)
      if (carU[0] != seed || carL[63] != seed) bad++;
      for (int l = 0; l < 64; l++) { prevU[l] = l > 0 ? own[l - 1] : prevU[0]; prevL[l] = l < 63 ? own[l + 1] : prevL[63]; }
      for (int l = 0; l < 64; l++) if (carU[l] != prevU[l] || carL[l] != prevL[l]) bad++;
    }
  }
  return bad;
}
extern "C" unsigned lds_exchange_bytes() { return 2u * 4u * pw::kOfferWords; }
'''

OTHER_HALVES = (0x0000, 0x0001, 0x7fff, 0x8000, 0xe000, 0xffff)        # (0xe000: -8192, the sentinel of the begin-anywhere rules)
NEGV = 0xe000e000

_LIB = {}


def _program(tmp_path_factory):
    if 'lib' not in _LIB:
        d = tmp_path_factory.mktemp('lds_exchange')
        src, so = os.path.join(str(d), 'offers.cpp'), os.path.join(str(d), 'liboffers.so')
        with open(src, 'w') as f:
            f.write(PROGRAM)
        subprocess.check_call(['g++', '-O1', '-std=c++17', '-shared', '-fPIC', '-I', CSRC, src, '-o', so])
        lib = ctypes.CDLL(so)
        lib.lds_exchange_check.restype = ctypes.c_uint
        lib.lds_exchange_bytes.restype = ctypes.c_uint
        _LIB['lib'] = lib
    return _LIB['lib']


@pytest.mark.parametrize('swap', [0, 1], ids=['low-half-runs', 'high-half-runs'])
@pytest.mark.parametrize('c', OTHER_HALVES, ids=['%04x' % c for c in OTHER_HALVES])
def test_host_forms_equal_the_expression_and_the_device_layout(c, swap, tmp_path_factory):
    lib = _program(tmp_path_factory)
    for seed in (NEGV, 0x12345678):
        first = (ctypes.c_uint * 9)()
        bad = lib.lds_exchange_check(c, swap, seed, 2, first)
        assert bad == 0, ('seed %08x' % seed, bad, 'first at half %04x, lane %d, round %d: up host %08x want %08x device %08x; '
                          'left host %08x want %08x device %08x' % tuple(first))


def test_the_two_arrays_are_520_bytes(tmp_path_factory):
    assert _program(tmp_path_factory).lds_exchange_bytes() == 520


CASES = PC.cases()


@pytest.mark.parametrize('case', CASES, ids=[c[0][0] for c in CASES])
def test_pair_key_cases_through_the_entry_points(case, oracle, form):       # noqa: F811
    PK._run_and_check(oracle, form, case, 1)
