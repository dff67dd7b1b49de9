"""LDS bank pattern of the ring kernel's pixel-fragment reads (csrc/conv_ring.hip), by enumeration: every
ds_read_b128 of a consumer wave must be conflict-free for all nine tap shifts, in the per-strip patch (row pitch 24
positions) and in the shared 2 x 2 tile patch (row pitch 42, strips at row offset 0 / 4 and column offset 0 / 20),
with the position swizzle (row & 1) << 1 on the 16-B channel piece."""
from collections import Counter

import pytest

# ds_read_b128 is served in four 16-lane groups (MI355X: bank = (byte address / 4) mod 64)
GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
          list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
GROUPS += [[lane + 32 for lane in g] for g in GROUPS]
POSB = 64  # bytes per patch position (32 bf16 channels)


def _worst_bank_use(pitch, strip_offsets, swizzle=True):
    worst = 0
    for roff, coff in strip_offsets:
        for ky in range(3):
            for kx in range(3):
                for blk in range(5):
                    for g in GROUPS:
                        banks = Counter()
                        for lane in g:
                            n, kq = lane & 15, lane >> 4
                            row, col = roff + (n >> 2) + ky, coff + 4 * blk + (n & 3) + kx
                            piece = kq ^ (((row & 1) << 1) if swizzle else 0)
                            a = (row * pitch + col) * POSB + piece * 16
                            banks.update(((a >> 2) + i) % 64 for i in range(4))
                        worst = max(worst, max(banks.values()))
    return worst


@pytest.mark.parametrize("pitch,offsets", [(24, [(0, 0)]), (42, [(0, 0), (0, 20), (4, 0), (4, 20)])])
def test_pixel_fragment_reads_are_conflict_free(pitch, offsets):
    assert _worst_bank_use(pitch, offsets) == 1


def test_swizzle_is_what_makes_them_conflict_free():
    assert _worst_bank_use(42, [(0, 0)], swizzle=False) > 1
