"""Shared inputs of the ``.geno`` export tests: a numpy statement of the table of
sai_amd/csrc/eigenstrat/geno_export.hpp, of the two packings and of the hash of the header record, and the int8 blocks
the host twin and the two kernels are run on.

``numpy_encode(block, ploidies, transposed)`` gives (records, status) for every slot of the block; the records of a
slot group of the transposed form are rows of it.  The unfit values are 3, -1 at ploidy 2, 2 at ploidy 1, 127 and
-128; the shapes are the sizes at which a record's length, a word of the packed kernel or a tile of the transposed one
changes."""

import numpy as np

BAD_INDEX = 0x7FFFFFFF
MIN_RECORD = 48
# dosage -> code (copies of the first allele, which is REF; 3 = missing), per ploidy
TABLE = {2: {0: 2, 1: 1, 2: 0, -2: 3}, 1: {0: 2, 1: 0, -1: 3}}
UNFIT = [(3, 2), (-1, 2), (2, 1), (127, 2), (-128, 2), (3, 1), (127, 1), (-128, 1)]
SLOT_COUNTS = [1, 3, 4, 5, 12, 13, 63, 64, 65, 191, 192, 193, 2002]  # rlen leaves 48 at 193
ROW_COUNTS = [1, 3, 4, 5, 15, 16, 17, 191, 192, 193, 255, 256, 257, 1000]  # 193: the transposed rlen leaves 48; 256: a tile


def record_bytes(n):
    return max(MIN_RECORD, -(-n // 4))


def hashit(name: bytes) -> int:
    h = 0
    for byte in name:
        h = (h * 23 + byte) & 0xFFFFFFFF
    return h


def hasharr(names) -> int:
    h = 0
    for name in names:
        h = ((h * 17) & 0xFFFFFFFF) ^ hashit(name if isinstance(name, bytes) else name.encode())
    return h


def codes_of(block, ploidies):
    """(codes uint8 [rows][slots], status int32 [rows]) by the table: what does not fit is 3 and is reported by its
    lowest slot; a ploidy outside 1 .. 2 is 3 in every row and every row says BAD_INDEX."""
    block = np.asarray(block, dtype=np.int8)
    n_rows, n_slots = block.shape
    pl = np.broadcast_to(np.asarray(ploidies, dtype=np.int64), (n_slots,))
    codes = np.full(block.shape, 3, dtype=np.uint8)
    fits = np.zeros(block.shape, dtype=bool)
    for ploidy, table in TABLE.items():
        for value, code in table.items():
            hit = (block == value) & (pl == ploidy)[None, :]
            codes[hit] = code
            fits |= hit
    first_bad = np.where((~fits).any(axis=1), n_slots - np.argmax(~fits, axis=1), 0).astype(np.int32)
    status = first_bad if np.isin(pl, (1, 2)).all() else np.full(n_rows, BAD_INDEX, dtype=np.int32)
    return codes, status


def pack_records(codes, rlen):
    """uint8 [records][fields] -> [records][rlen]: the first field of a byte in its two most significant bits."""
    padded = np.zeros((codes.shape[0], rlen * 4), dtype=np.uint8)
    padded[:, : codes.shape[1]] = codes
    q = padded.reshape(codes.shape[0], rlen, 4)
    return (q[:, :, 0] << 6 | q[:, :, 1] << 4 | q[:, :, 2] << 2 | q[:, :, 3]).astype(np.uint8)


def numpy_encode(block, ploidies, transposed=False):
    codes, status = codes_of(block, ploidies)
    n_rows, n_slots = codes.shape
    if transposed:
        return pack_records(np.ascontiguousarray(codes.T), record_bytes(n_rows)), status
    return pack_records(codes, record_bytes(n_slots)), status


def random_block(rng, n_rows, n_slots, ploidies):
    """Values of the table only, every cell of it likely."""
    pl = np.broadcast_to(np.asarray(ploidies), (n_slots,))
    dip = rng.choice(np.array([2, 1, 0, -2], dtype=np.int8), size=(n_rows, n_slots))
    hap = rng.choice(np.array([1, 0, -1], dtype=np.int8), size=(n_rows, n_slots))
    return np.where((pl == 2)[None, :], dip, hap).astype(np.int8)


def ploidy_cases(rng, n_slots):
    mixed = rng.integers(1, 3, n_slots).astype(np.int32)
    mixed[0], mixed[n_slots - 1] = 1, 2  # never uniform, unless there is one slot
    return [("uniform 2", 2), ("uniform 1", 1), ("per slot", mixed)]


def table_block():
    """Every cell of the table at both ploidies, per-slot: slots 0 .. 3 diploid with 0, 1, 2, -2 and slots 4 .. 6 haploid
    with 0, 1, -1, the values rotated row by row among the slots of their ploidy."""
    pl = np.array([2, 2, 2, 2, 1, 1, 1], dtype=np.int32)
    dip, hap = [0, 1, 2, -2], [0, 1, -1]
    block = np.array([[dip[(k + r) % 4] for k in range(4)] + [hap[(k + r) % 3] for k in range(3)] for r in range(12)], dtype=np.int8)
    return block, pl


def plant_unfit(rng, block, ploidies):
    """Values outside the table in about one row of three: one somewhere, or at the first, a middle and the last slot
    (the lowest is reported).  -> the block, changed in place"""
    n_rows, n_slots = block.shape
    pl = np.broadcast_to(np.asarray(ploidies), (n_slots,))
    for r in range(0, n_rows, 3):
        for where in {0, n_slots // 2, n_slots - 1} if r % 2 else {int(rng.integers(n_slots))}:
            choices = [v for v, p in UNFIT if p == pl[where]]
            block[r, where] = choices[int(rng.integers(len(choices)))]
    return block


def shapes():
    """(n_rows, n_slots) that reach every slot count and every row count without the full product: every slot count at
    three row counts, every row count at three slot counts."""
    out = [(r, s) for s in SLOT_COUNTS for r in (1, 17, 257)] + [(r, s) for r in ROW_COUNTS for s in (5, 65, 193)]
    out += [(1000, 2002), (193, 2002)]
    return sorted(set(out))


def slot_groups(n_slots):
    """(slot0, n_out) choices of the transposed form: everything, one slot only, a group that starts and ends inside a
    64-slot tile, and one that spans more than one tile."""
    groups = [(0, n_slots), (n_slots - 1, 1), (n_slots // 2, 1)]
    if n_slots >= 8:
        groups.append((3, min(n_slots - 3, 40)))
    if n_slots >= 100:
        groups.append((7, min(n_slots - 7, 150)))
    return sorted(set(groups))
