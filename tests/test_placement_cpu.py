"""tests/placement_cases.py proven from the addresses alone: the arena always holds its two points with room on each
side, and every kind of placement has the property its name promises."""
import pytest

import placement_cases as PC

BIT31 = 1 << 31
G4 = 1 << 32
# (nbytes, row_bytes): the operands of tests/test_gpu_placement.py by size and row -- A [4100, 128] fp16 (a row is 256
# bytes: every multiple of 256 is a row boundary), A [4100, 192] bf16, split8 A [4100, 256], W [256, 128], fp32 out
# [4100, 256], packed qkv rows of B = 2, H = 2 at L = 600 and 130 (16-bit, split16 and qk8 records), x segments, and a
# one-row vector
SIZES = [(4100 * 256, 256), (4100 * 384, 384), (4100 * 1024, 1024), (256 * 256, 256), (4100 * 1024, 1024),
         (1200 * 768, 768), (260 * 768, 768), (1200 * 1536, 1536), (1200 * 1280, 1280), (64 * 1536, 1536), (1024, 0),
         (37 * 1536, 1536), (512, 128), (32, 32)]


def bases():
    """every 2 MiB-aligned base over a span of more than 4 GiB starting high in the address space, and the worst cases
    next to the multiples of 2^32 and 2^31"""
    start = 0x7F00 << 32
    out = [start + i * 2 * PC.MIB for i in range((G4 + 64 * PC.MIB) // (2 * PC.MIB))]
    for k in (start, start + BIT31):
        for d in (-2 * PC.MIB, 0, 2 * PC.MIB):
            for m in (0, PC.MARGIN):
                out.append(k - m + d)
    return out


def test_arena_always_holds_both_points_with_room():
    n = 0
    for base in bases():
        T, U = PC.arena_points(base, PC.ARENA_BYTES)
        end = base + PC.ARENA_BYTES
        assert T % G4 == 0 and T >= base + PC.MARGIN and T - G4 < base + PC.MARGIN          # the smallest such multiple
        assert abs(U - T) == BIT31 and U % BIT31 == 0 and U % G4 != 0
        for pnt in (T, U):
            assert pnt - base >= PC.MARGIN and end - pnt >= PC.MARGIN
        assert (U < T) == (T - BIT31 - base >= PC.MARGIN)                                   # below T whenever it fits
        n += 1
    assert n > 2048


def test_arena_points_refuses_an_arena_that_is_too_small():
    with pytest.raises(AssertionError):
        PC.arena_points(G4 - 2 * PC.MIB, 4 * PC.GIB)


@pytest.mark.parametrize("base", [0x7F00 << 32, (0x7F00 << 32) + BIT31 - 2 * PC.MIB, (0x7F01 << 32) - PC.MARGIN + 2 * PC.MIB])
def test_every_kind_of_placement_keeps_its_promise(base):
    T, U = PC.arena_points(base, PC.ARENA_BYTES)
    end = base + PC.ARENA_BYTES
    for nbytes, row in SIZES:
        spans = []
        for slot in range(PC.MAX_SLOT + 1):
            a = PC.place(nbytes, "high", T, U, slot, row)
            assert a % PC.ALIGN == 0 and a + nbytes <= T - slot * PC.LANE - PC.ALIGN < a + nbytes + PC.ALIGN
            assert a & BIT31 and (a + nbytes - 1) & BIT31 and a >> 32 == (a + nbytes - 1) >> 32    # bit 31 set throughout
            spans.append((a, a + nbytes))
            b = PC.place(nbytes, "low", T, U, slot, row)
            assert b == T + slot * PC.LANE and b % PC.ALIGN == 0 and (b & (G4 - 1)) == slot * PC.LANE
            assert not (b + nbytes - 1) & BIT31
            spans.append((b, b + nbytes))
        if nbytes > 32:
            for kind, pnt in (("cross4g", T), ("cross2g", U)):
                c = PC.place(nbytes, kind, T, U, 0, row)
                assert c < pnt < c + nbytes and c % 16 == 0
                assert c % PC.ALIGN == 0 or (row and PC.ALIGN % row == 0 and c % (row // 2) == 0)
                if row:
                    assert (pnt - c) % row != 0                      # the point is inside a row
                    first, last = c, c + (nbytes // row - 1) * row   # addresses of the first and the last row
                    if kind == "cross4g":
                        assert first >> 32 != last >> 32 and first & BIT31 and not last & BIT31
                    else:
                        assert bool(first & BIT31) != bool(last & BIT31)
                spans.append((c, c + nbytes))
        # inside the arena with their guards; the slots do not touch one another, and a crossing tensor (which has the
        # lane around its point to itself) touches no slot from 1 on
        for lo, hi in spans:
            assert base <= lo - PC.GUARD and hi + PC.GUARD <= end
        slots, crossing = spans[:2 * (PC.MAX_SLOT + 1)], spans[2 * (PC.MAX_SLOT + 1):]
        high, low = slots[0::2], slots[1::2]                 # a run is all high, all low, or one crossing + high slots
        for group in (high, low, high[1:] + crossing):
            padded = sorted((lo - PC.GUARD, hi + PC.GUARD) for lo, hi in group)
            for (_, h0), (l1, _) in zip(padded, padded[1:]):
                assert h0 <= l1


def test_runs_cover_what_the_cases_need():
    ops = [("A", "desc"), ("W", "desc"), ("bias", "in"), ("out", "out")]
    rs = dict(PC.runs(ops))
    assert list(rs) == ["all_high", "all_low", "A_cross4g", "A_cross2g", "W_cross4g", "W_cross2g", "out_cross4g"]
    assert {k for k, _ in rs["all_high"].values()} == {"high"} and {k for k, _ in rs["all_low"].values()} == {"low"}
    for name, m in rs.items():
        assert set(m) == {"A", "W", "bias", "out"}
        slots = [(k, s) for k, s in m.values() if k in ("high", "low")]
        assert len(slots) == len(set(slots)) and all(s <= PC.MAX_SLOT for _, s in slots)      # no two operands share a slot
        crossing = [n for n, (k, _) in m.items() if k.startswith("cross")]
        assert len(crossing) == (0 if name.startswith("all_") else 1)
        if crossing:                                         # the lane around T belongs to the crossing operand
            assert all(s >= 1 for n, (k, s) in m.items() if n not in crossing)
