"""CPU: the index arithmetic of the LDS-staged epilogue of wino4_fused2_kernel (csrc/wn_wino.hip), restated in numpy.

One output's conditioning tile is 32 rows x 64 columns (tanh half | sigmoid half).  Request k of a wave lands lane l's 16 bytes
at byte 1024 k + 16 l of the slot; the lane chooses WHICH row and 16-byte piece of the plane it fetches.  The accumulator layout
reads the tile back 4 bytes per lane, writes the gated value over its tanh element, and the store pass reads rows back 16
bytes per lane.  Every element must be written once and read from where it was written, and no access may conflict on banks.

The three maps below are written out here by hand (division and remainder, no bit tricks), independently of the kernel's
constexpr functions; the last test reads those functions' return expressions from the source and checks that they are the same
maps over their whole domain (it depends on the one-line form of the three functions; if they are reformatted it fails with
"not found" and is to be adjusted, the maps here are not).
"""
import os
import re

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'text_to_speech_amd', 'csrc', 'wn_wino.hip')


def stage_row(k, lane):
    """Tile row that lane `lane` fetches with request k: four rows per request, 16 lanes per row."""
    return 4 * k + lane // 16


def stage_piece(lane):
    """16-byte piece of that row the lane fetches: its own, but in the rows of the upper half wave (rows 2, 3 of the four:
    the rows with bit 1 set) the two 128-byte halves change places."""
    piece = lane % 16
    return (piece + 8) % 16 if lane // 32 == 1 else piece


def stage_at(row, col):
    """Float offset in the slot of tile element (row, col): rows are 64 floats; rows 2, 3 mod 4 keep their halves swapped."""
    swapped = (row // 2) % 2 == 1
    return row * 64 + ((col + 32) % 64 if swapped else col)


def _staged_slot(plane):
    """The slot after the eight requests of a wave (floats), and how often every float was written."""
    slot = np.full(32 * 64, np.nan)
    hits = np.zeros(32 * 64, int)
    for k in range(8):
        for lane in range(64):
            row, piece = stage_row(k, lane), stage_piece(lane)
            assert 0 <= row < 32 and 0 <= piece < 16
            dst = 256 * k + 4 * lane                                   # wave-uniform base + 16 bytes per lane
            slot[dst:dst + 4] = plane[row, 4 * piece:4 * piece + 4]
            hits[dst:dst + 4] += 1
    return slot, hits


def test_every_element_of_the_tile_is_written_once_and_read_where_it_was_written():
    plane = np.arange(32 * 64, dtype=float).reshape(32, 64)
    slot, hits = _staged_slot(plane)
    assert (hits == 1).all() and sorted(slot) == sorted(plane.ravel())
    gated = -1.0 - plane[:, :32]
    seen = np.zeros((32, 64), int)
    for lane in range(64):
        li, lh = lane & 31, lane >> 5
        mine = lh * (4 * 64) + li                                      # the kernel's per-lane base
        for r in range(16):
            row0 = (r & 3) + 8 * (r >> 2)
            t, s = mine + stage_at(row0, 0), mine + stage_at(row0, 32)
            assert t == stage_at(row0 + 4 * lh, li) and s == stage_at(row0 + 4 * lh, 32 + li)
            assert slot[t] == plane[row0 + 4 * lh, li] and slot[s] == plane[row0 + 4 * lh, 32 + li]
            seen[row0 + 4 * lh, li] += 1
            seen[row0 + 4 * lh, 32 + li] += 1
            slot[t] = gated[row0 + 4 * lh, li]                         # in place of the consumed tanh element
    assert (seen == 1).all()
    for lane in range(64):                                             # the store pass: 16 bytes of one row per lane
        er, ec4 = lane >> 3, (lane & 7) * 4
        for qq in range(4):
            o = (er + 8 * qq) * 64 + (((er >> 1) & 1) << 5) + ec4
            assert (slot[o:o + 4] == gated[er + 8 * qq, ec4:ec4 + 4]).all()


def test_no_access_of_the_epilogue_conflicts_on_lds_banks():
    # 4-byte reads and writes: bank = dword % 32 inside each half of the wave
    for r in range(16):
        row0 = (r & 3) + 8 * (r >> 2)
        for lh in range(2):
            for col0 in (0, 32):
                banks = {(lh * 256 + li + stage_at(row0, col0)) % 32 for li in range(32)}
                assert len(banks) == 32
    # 16-byte reads: bank = dword % 64 inside each of the four lane groups of ds_read_b128
    groups = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
              list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
    groups += [[l + 32 for l in g] for g in groups]
    for qq in range(4):
        for g in groups:
            banks = set()
            for lane in g:
                er, ec4 = lane >> 3, (lane & 7) * 4
                o = (er + 8 * qq) * 64 + (((er >> 1) & 1) << 5) + ec4
                banks |= {(o + i) % 64 for i in range(4)}
            assert len(banks) == 64


def _source_expr(name):
    src = open(SRC).read()
    m = re.search(r'constexpr int %s\(([^)]*)\) \{ return (.*?); \}' % name, src)
    assert m, f'{name} not found in wn_wino.hip as a one-line constexpr function'
    assert '/' not in m.group(2) and '%' not in m.group(2)             # (C and Python agree on + - * ^ & << >> of non-negatives)
    args = [a.split()[-1] for a in m.group(1).split(',')]
    return eval('lambda %s: %s' % (', '.join(args), m.group(2)))


def test_the_kernels_constexpr_maps_are_the_maps_restated_here():
    k_row, k_piece, k_at = _source_expr('wino_stage_row'), _source_expr('wino_stage_piece'), _source_expr('wino_stage_at')
    for lane in range(64):
        assert k_piece(lane) == stage_piece(lane)
        for k in range(8):
            assert k_row(k, lane) == stage_row(k, lane)
    for row in range(32):
        for col in range(64):
            assert k_at(row, col) == stage_at(row, col)
