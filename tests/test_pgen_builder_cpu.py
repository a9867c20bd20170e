"""tests/pgen_builder.py against bytes worked out by hand: the worked example of DESIGN_INGEST.md ("PLINK 2
filesets"), committed as hex text, and the varints and the layout of a difflist at its group boundaries."""

import numpy as np

import pgen_builder as B
from conftest import ROOT

EXAMPLE_CODES = [[0, 1, 2, 3, 1], [0, 0, 0, 2, 0], [0, 1, 0, 2, 0], [2, 2, 3, 2, 0], [0, 0, 3, 1, 2]]
EXAMPLE_TYPES = [0, 4, 2, 1, 3]


def example_bytes() -> bytes:
    return B.parse_hex((ROOT / "tests" / "golden" / "pgen_worked_example.hex").read_text())


def test_the_worked_example_is_reproduced_byte_for_byte():
    want = example_bytes()
    assert len(want) == 44 and want[:3] == b"\x6c\x1b\x10" and want[-3:] == b"\x01\x03\x01"
    data, table = B.build_pgen(EXAMPLE_CODES, EXAMPLE_TYPES)
    assert data == want
    assert table == [(28, 2, 0, -1), (30, 3, 4, -1), (33, 3, 2, 1), (36, 5, 1, -1), (41, 3, 3, 3)]
    # the smallest encoding is never longer than the forced one, and decodes to the same thing elsewhere (test_pgen_cpu)
    smallest, small_table = B.build_pgen(EXAMPLE_CODES)
    assert len(smallest) <= len(want) and [t[1] for t in small_table] <= [t[1] for t in table]


def test_varints():
    assert B.varint(0) == b"\x00" and B.varint(1) == b"\x01" and B.varint(127) == b"\x7f"
    assert B.varint(128) == b"\x80\x01" and B.varint(300) == b"\xac\x02" and B.varint(16383) == b"\xff\x7f"
    assert B.varint(16384) == b"\x80\x80\x01" and B.varint(65536) == b"\x80\x80\x04"
    assert [B.index_width(n) for n in (1, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24)] == [1, 1, 2, 2, 3, 3, 4]


def test_difflist_layout_at_the_group_boundaries():
    # L = 0: the length alone
    assert B.difflist([], [], 5) == b"\x00"
    # L = 1: length, one first index, no size byte, one code byte, no deltas
    assert B.difflist([3], [2], 5) == b"\x01\x03\x02"
    assert B.difflist([300], [1], 1000) == b"\x01\x2c\x01\x01"  # two-byte index from 256 samples on
    # L = 64: one group; 63 deltas of 2 -> one byte each; 16 code bytes of 01 10 11 00 ... = 0x39 (k mod 4 -> 1, 2, 3, 0)
    samples = list(range(5, 5 + 2 * 64, 2))
    codes = [(k + 1) % 4 for k in range(64)]
    got = B.difflist(samples, codes, 200)
    assert got == b"\x40" + b"\x05" + bytes([1 | 2 << 2 | 3 << 4 | 0 << 6]) * 16 + b"\x02" * 63
    # L = 65: two groups; the first group's size byte is 63 - 63 = 0; the second group has a first index and no delta
    samples.append(199)
    got = B.difflist(samples, codes + [3], 200)
    assert got == b"\x41" + bytes([5, 199]) + b"\x00" + bytes([0x39]) * 16 + b"\x03" + b"\x02" * 63
    # a two-byte delta makes the size byte 1, and three-byte deltas appear from 16 384 on
    wide = [0] + [200 + k for k in range(62)] + [500, 40000, 65536]
    L, firsts, sizes, code_bytes, deltas = B.difflist_parts(wide, [1] * 66, 65537)
    assert L == b"\x42" and firsts == (0).to_bytes(3, "little") + (40000).to_bytes(3, "little") and sizes == bytes([2])
    assert deltas[0] == b"\xc8\x01" + b"\x01" * 61 + b"\xef\x01" and len(deltas[0]) == 65 and deltas[1] == b"\xc0\xc7\x01"
    assert len(code_bytes) == 17


def test_every_type_round_trips_through_a_plain_decoder():
    """A decoder of a dozen lines, written here from the same rules: what the builder writes means what was asked."""

    def read_varint(buf, at):
        value = shift = 0
        while True:
            value |= (buf[at] & 127) << shift
            shift += 7
            at += 1
            if not buf[at - 1] & 128:
                return value, at

    def apply(buf, at, row):
        n = len(row)
        L, at = read_varint(buf, at)
        if L == 0:
            return
        G, w = -(-L // 64), B.index_width(n)
        firsts, sizes = at, at + G * w
        code_at = sizes + G - 1
        d = code_at + -(-L // 4)
        for g in range(G):
            s = int.from_bytes(buf[firsts + g * w : firsts + (g + 1) * w], "little")
            for j in range(min(64, L - 64 * g)):
                if j:
                    delta, d = read_varint(buf, d)
                    s += delta
                k = 64 * g + j
                row[s] = buf[code_at + k // 4] >> 2 * (k % 4) & 3

    def decode(buf, kind, n, base):
        if kind == 0:
            return np.array([buf[i // 4] >> 2 * (i % 4) & 3 for i in range(n)], dtype=np.uint8)
        if kind == 1:
            lo, hi = buf[0] // 4, buf[0] // 4 + (buf[0] & 3)
            row = np.array([hi if buf[1 + i // 8] >> i % 8 & 1 else lo for i in range(n)], dtype=np.uint8)
            apply(buf, 1 + -(-n // 8), row)
            return row
        row = {2: lambda: base.copy(), 3: lambda: B.swap02(base), 4: lambda: np.zeros(n, np.uint8), 6: lambda: np.full(n, 2, np.uint8),
               7: lambda: np.full(n, 3, np.uint8)}[kind]()  # fmt: skip
        apply(buf, 0, row)
        return row

    rng = np.random.default_rng(11)
    for n in (1, 5, 64, 300):
        base = rng.integers(0, 4, n).astype(np.uint8)
        for density in (0.0, 0.02, 0.6):
            row = base.copy()
            hit = rng.random(n) < density
            row[hit] = rng.integers(0, 4, int(hit.sum()))
            for kind in (0, 1, 2, 3, 4, 6, 7):
                assert np.array_equal(decode(B.encode(row, kind, base), kind, n, base), row), (n, density, kind)
