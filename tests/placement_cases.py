"""Where the operands of the descriptor-building kernels are put (tests/test_gpu_placement.py): pure functions of
addresses, proven on the CPU by tests/test_placement_cpu.py.

A kernel that rebuilds a buffer-descriptor base from the halves of a 64-bit address can go wrong in three places: the
low half has bit 31 set (a signed low half sign-extends), the low half wraps inside the tensor (a 4 GiB boundary falls
in it), or bit 31 flips inside the tensor.  One arena of 4 GiB + 512 MiB always holds a 4 GiB boundary T and a point
U = T -+ 2 GiB with 256 MiB of arena on each side of both, whatever base the allocator hands out."""
GIB = 1 << 30
MIB = 1 << 20
ARENA_BYTES = 4 * GIB + 512 * MIB
MARGIN = 256 * MIB            # arena on each side of T and of U
ALIGN = 256
GUARD = 4096                  # guard bytes on each side of a placed output
LANE = 64 * MIB               # distance between the slots of one kind; a tensor and its guards fit in one lane
MAX_SLOT = 3
KINDS = ("high", "low", "cross4g", "cross2g")


def arena_points(base: int, size: int):
    """-> (T, U): T the smallest multiple of 2^32 >= base + 256 MiB; U = T - 2^31 when that leaves 256 MiB of arena
    below it, else T + 2^31"""
    T = (base + MARGIN + (1 << 32) - 1) >> 32 << 32
    U = T - (1 << 31)
    if U - base < MARGIN:
        U = T + (1 << 31)
    assert base + MARGIN <= T <= base + size - MARGIN and base + MARGIN <= U <= base + size - MARGIN, (base, size)
    return T, U


def cross_offset(nbytes: int, row_bytes: int):
    """-> (offset, alignment): how far in front of the crossing point a tensor starts, so that the point falls strictly
    inside it and not on a row boundary.  The offset is a multiple of 256 near the middle; where every multiple of 256
    is a row boundary (row_bytes divides 256) the alignment drops to half a row, 16 bytes at the least."""
    align = ALIGN
    if row_bytes and ALIGN % row_bytes == 0:
        align = row_bytes // 2
        assert align >= 16 and align % 16 == 0, row_bytes
    off = nbytes // 2 // align * align
    if off == 0:
        off = align
    if row_bytes and off % row_bytes == 0:
        off += align
    assert 0 < off < nbytes and (not row_bytes or off % row_bytes), (nbytes, row_bytes)
    return off, align


def place(nbytes: int, kind: str, T: int, U: int, slot: int = 0, row_bytes: int = 0) -> int:
    """-> the address of a tensor of nbytes.
    high     the whole tensor has bit 31 set; slot 0 ends 256 bytes below T, slot k one LANE further down each
    low      starts at T (slot k: T + k LANE): the low half of the address is near 0
    cross4g  T falls strictly inside the tensor and not on a row boundary
    cross2g  U falls strictly inside: bit 31 differs between rows of the same tensor
    256-byte aligned (the crossing kinds: see cross_offset).  Only one operand of a call crosses, so those take no slot."""
    assert 0 < nbytes <= LANE - 2 * GUARD - ALIGN and 0 <= slot <= MAX_SLOT and kind in KINDS
    if kind == "high":
        return (T - ALIGN - slot * LANE - nbytes) // ALIGN * ALIGN
    if kind == "low":
        return T + slot * LANE
    off, _ = cross_offset(nbytes, row_bytes)
    return (T if kind == "cross4g" else U) - off


def runs(operands):
    """operands: [(name, role)], role 'desc' (read through a buffer descriptor), 'in' or 'out' -> the placement runs of
    a case, each {name: (kind, slot)}: all high; all low; every 'desc' operand cross4g and cross2g with the others
    high; every output cross4g once (the others high)"""
    names = [n for n, _ in operands]
    out = [("all_high", {n: ("high", i) for i, n in enumerate(names)}),
           ("all_low", {n: ("low", i) for i, n in enumerate(names)})]

    def one_crossing(which, kind):
        rest = [n for n in names if n != which]
        m = {n: ("high", i + 1) for i, n in enumerate(rest)}
        m[which] = (kind, 0)
        return m
    for n, role in operands:
        if role == "desc":
            out.append((f"{n}_cross4g", one_crossing(n, "cross4g")))
            out.append((f"{n}_cross2g", one_crossing(n, "cross2g")))
    for n, role in operands:
        if role == "out":
            out.append((f"{n}_cross4g", one_crossing(n, "cross4g")))
    return out
