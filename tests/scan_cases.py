"""Inputs and numpy statements for the list bookkeeping of the windows stage (window_scan_partials_kernel,
window_scan_apply_kernel and the -1 / capacity handling of window_lists_kernel in sai_amd/csrc/windows.hip) and for
the one-workgroup scan behind sai_text_line_starts (scan_blocks_kernel in sai_amd/csrc/lines.hip).  Plain numpy:
test_scan_cases_cpu.py pins the statements to the oracle and checks that every case is what it says,
test_window_lists_device.py and test_line_scan_device.py run the kernels.

Window cases: one small block of sites, many overlapping windows of K consecutive sites handed over as lo / hi
arrays, so that hundreds of thousands of records cost next to nothing to compute -- what is under test is the
scan over the records' list sizes, not the statistics.  The block is designed so that every set has a condition
site in every window:
  * sites i % 3 == 0 have an all-zero reference and source 0 fixed (tight set A: w = 0.3, source 0 "= 1");
  * sites i % 3 == 1 the same with source 1 (tight set B);
  * of the sites i % 3 == 2 half have a fixed reference (frequency 1 = w of the loose sets: no condition site), and
    reference individual 0 never carries the allele at the others;
  * sites i % 7 == 0 have both sources fixed: the one set without ancestral alleles inverts them.
"""

from __future__ import annotations

import operator
import zlib
from dataclasses import dataclass
from functools import lru_cache
from pathlib import Path

import numpy as np

from capacity_cases import parse_constants

CSRC = Path(__file__).resolve().parent.parent / "sai_amd" / "csrc"
K = 6  # sites per window
PLOIDY = (2, 2, 2, 2)
CANARY = -0x21524111  # int32 filler of the list buffers: never a position
MAX_SETS = 20


@lru_cache(maxsize=None)
def scan_block() -> int:
    """Records per workgroup of the two scan kernels, from the source."""
    return parse_constants((CSRC / "windows.hip").read_text())["kScanBlock"]


@lru_cache(maxsize=None)
def scan_threads() -> int:
    return parse_constants((CSRC / "windows.hip").read_text())["kScanThreads"]


def scan_grid(records: int) -> int:
    return -(-records // scan_block())


def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- the block --------------------------------------------------------------------------------------


@dataclass(frozen=True)
class Block:
    mats: tuple  # ref, tgt, source 0, source 1: int8 [n_sites][n_ind]
    pos: np.ndarray  # int64, ascending


@lru_cache(maxsize=None)
def block(name: str, n_sites: int, missing: float = 0.0) -> Block:
    rng = _rng(name)
    p = rng.random(n_sites)
    ref = rng.binomial(2, 0.6 * p[:, None], size=(n_sites, 6)).astype(np.int8)
    tgt = rng.binomial(2, p[:, None], size=(n_sites, 7)).astype(np.int8)
    src0 = rng.binomial(2, p[:, None], size=(n_sites, 3)).astype(np.int8)
    src1 = rng.binomial(2, p[:, None], size=(n_sites, 2)).astype(np.int8)
    i = np.arange(n_sites)
    ref[:, 0] = 0
    ref[i % 3 == 0] = 0
    src0[i % 3 == 0] = 2
    ref[i % 3 == 1] = 0
    src1[i % 3 == 1] = 2
    src0[i % 7 == 0] = 2
    src1[i % 7 == 0] = 2
    ref[(i % 3 == 2) & (rng.random(n_sites) < 0.5)] = 2  # reference frequency 1: no condition site of any set
    if missing:
        for m in (ref, tgt, src0, src1):
            m[rng.random(m.shape) < missing] = -1
        for m, sites in ((tgt, (5, 40)), (ref, (11,)), (src1, (17, 18))):  # nothing called: the frequency is NaN
            m[list(sites)] = -1
        ref[100:110] = -1  # a stretch in which no set has a condition site
    pos = 100 + np.cumsum(rng.integers(1, 9, n_sites)).astype(np.int64)
    return Block((ref, tgt, src0, src1), pos)


LOOSE = ((">=", 0.0), (">=", 0.0))
TIGHT_A = (("=", 1.0), (">=", 0.0))
TIGHT_B = ((">=", 0.0), ("=", 1.0))


def _spec(w, x, quantile, y, anc=True):
    return dict(w=float(w), x=float(x), quantile=float(quantile), y_list=list(y), anc=bool(anc))


POOL = (
    _spec(1.0, 0.5, 0.95, LOOSE), _spec(1.0, 0.0, 0.5, LOOSE), _spec(0.3, 0.2, 1.0, TIGHT_A), _spec(1.0, 0.9, 0.0, LOOSE),
    _spec(1.0, 0.3, 0.5, LOOSE, anc=False), _spec(0.5, 0.0, 0.0, TIGHT_B), _spec(1.0, 0.2, 0.3, LOOSE), _spec(1.0, 1.0, 0.777, LOOSE),
    _spec(0.3, 0.6, 0.5, TIGHT_A), _spec(1.0, 0.7, 1.0, LOOSE), _spec(1.0, 0.1, 0.05, LOOSE), _spec(1.0, 0.4, 0.25, LOOSE),
    _spec(1.0, 0.6, 0.75, LOOSE), _spec(0.5, 0.5, 0.9, TIGHT_B), _spec(1.0, 0.8, 0.99, LOOSE), _spec(1.0, 0.25, 0.0, LOOSE),
    _spec(1.0, 0.35, 1.0, LOOSE), _spec(1.0, 0.45, 0.5, LOOSE), _spec(1.0, 0.55, 0.6, LOOSE), _spec(1.0, 0.65, 0.4, LOOSE),
)  # fmt: skip
assert len(POOL) == MAX_SETS


# ---- the numpy statement ------------------------------------------------------------------------------

_COMPARE = {"=": operator.eq, "<": operator.lt, ">": operator.gt, "<=": operator.le, ">=": operator.ge}


def site_freq(g: np.ndarray, ploidy: int) -> np.ndarray:
    """sum / (called * ploidy) in float64, NaN where nothing is called."""
    present = g >= 0
    total = np.where(present, g, 0).sum(axis=1).astype(np.float64)
    denom = (present.sum(axis=1) * ploidy).astype(np.float64)
    out = np.full(g.shape[0], np.nan)
    np.divide(total, denom, out=out, where=denom > 0)
    return out


def site_level(blk: Block, spec: dict):
    """(condition, effective target frequency) per site of one parameter set, by plain comparisons."""
    ref, tgt, *srcs = [site_freq(m.astype(np.int64), p) for m, p in zip(blk.mats, PLOIDY)]
    valid = np.ones(ref.shape, dtype=bool)
    for f in (ref, tgt, *srcs):
        valid &= np.isfinite(f) & (f >= 0) & (f <= 1)
    with np.errstate(invalid="ignore"):
        hits = np.ones(ref.shape, dtype=bool)
        for f, (op, y) in zip(srcs, spec["y_list"]):
            hits &= _COMPARE[op](f, y)
        if not spec["anc"]:
            mirror = np.ones(ref.shape, dtype=bool)
            for f, (op, y) in zip(srcs, spec["y_list"]):
                mirror &= _COMPARE[op](f, 1 - y)
            flip = mirror & valid
            ref, tgt = np.where(flip, 1 - ref, ref), np.where(flip, 1 - tgt, tgt)
            hits |= mirror
        return valid & hits & (ref < spec["w"]), tgt


@dataclass
class WindowCase:
    name: str
    blk: Block
    specs: list
    lo: np.ndarray  # int32 [n_windows]
    hi: np.ndarray
    large: bool  # no missing calls: every record has condition sites

    @property
    def n_sets(self) -> int:
        return len(self.specs)

    @property
    def n_windows(self) -> int:
        return int(self.lo.size)

    @property
    def records(self) -> int:
        return self.n_sets * self.n_windows

    @property
    def form(self) -> str:
        return "shared" if self.n_sets >= 4 else "wave"  # kWinWaves sets and more: one workgroup per window

    @property
    def grid(self) -> int:
        return scan_grid(self.records)


@dataclass
class Reference:
    """Per record in (set, window) order; the lists of all records behind each other."""

    n_sites: np.ndarray
    n_cond: np.ndarray
    u_count: np.ndarray
    n_cdd_q: np.ndarray
    q: np.ndarray
    u_flat: np.ndarray  # int32 positions, ascending site order inside a record
    q_flat: np.ndarray

    def counts(self, which: int) -> np.ndarray:
        return (self.u_count, self.n_cdd_q)[which].astype(np.int64)

    def flat(self, which: int) -> np.ndarray:
        return (self.u_flat, self.q_flat)[which]

    def need(self, which: int) -> int:
        return int(self.counts(which).sum())

    def list_of(self, which: int, record: int) -> np.ndarray:
        c = self.counts(which)
        a = int(c[:record].sum())
        return self.flat(which)[a : a + int(c[record])]


def _row_quantile(f: np.ndarray, cond: np.ndarray, quantile: float) -> np.ndarray:
    """np.quantile (default method 'linear') of every row's selected values; NaN for a row that selects none.
    Rows are grouped by how many values they select, each group is a matrix reduced along axis 1."""
    n_sel = cond.sum(axis=1)
    order = np.argsort(~cond, axis=1, kind="stable")  # the selected values first, in site order
    front = np.take_along_axis(f, order, axis=1)
    out = np.full(f.shape[0], np.nan)
    for c in np.unique(n_sel):
        if c:
            rows = np.flatnonzero(n_sel == c)
            out[rows] = np.quantile(front[rows, :c], quantile, axis=1)
    return out


@lru_cache(maxsize=6)  # a large case's reference is some 20 MB: the last few stay, tests take the cases in order
def _reference(name: str) -> Reference:
    case = window_case(name)
    sites = case.lo.astype(np.int64)[:, None] + np.arange(K)[None, :]  # [n_windows][K]
    assert np.array_equal(sites[:, -1] + 1, case.hi)
    pos32 = case.blk.pos.astype(np.int32)
    n_cond, u_count, n_q, qs, u_parts, q_parts = [], [], [], [], [], []
    for spec in case.specs:
        cond_site, eff_site = site_level(case.blk, spec)
        cond, f = cond_site[sites], eff_site[sites]
        with np.errstate(invalid="ignore"):
            in_u = cond & (f > spec["x"])
            q = _row_quantile(f, cond, spec["quantile"])
            in_q = cond & (f >= q[:, None])
        n_cond.append(cond.sum(axis=1))
        u_count.append(in_u.sum(axis=1))
        n_q.append(in_q.sum(axis=1))
        qs.append(q)
        u_parts.append(pos32[sites[in_u]])  # row-major: record order, ascending sites inside a record
        q_parts.append(pos32[sites[in_q]])
    cat = np.concatenate
    return Reference(np.full(case.records, K, dtype=np.int64), cat(n_cond), cat(u_count), cat(n_q), cat(qs), cat(u_parts), cat(q_parts))


def reference(case: WindowCase) -> Reference:
    """Shared by the tests that use a case one after the other; callers leave it unchanged."""
    return _reference(case.name)


def expected_offsets(counts: np.ndarray, cap: int) -> np.ndarray:
    """Start of every record's list: the exclusive running sum of the counts, -1 where offset + count > cap."""
    counts = counts.astype(np.int64)
    off = np.cumsum(counts) - counts
    return np.where(off + counts <= cap, off, -1)


def expected_partials(counts: np.ndarray) -> np.ndarray:
    """The sum of every scan workgroup's records."""
    pad = np.zeros(scan_grid(counts.size) * scan_block(), dtype=np.int64)
    pad[: counts.size] = counts
    return pad.reshape(-1, scan_block()).sum(axis=1)


def expected_region(flat: np.ndarray, counts: np.ndarray, cap: int) -> np.ndarray:
    """The cap words of a list buffer after the call: the lists of the records that fit where their offsets put
    them, the canary in every other word."""
    off = expected_offsets(counts, cap)
    out = np.full(cap, CANARY, dtype=np.int32)
    owned = np.repeat(off >= 0, counts)  # per entry of the flat list: its record fits
    at = np.flatnonzero(owned)  # offsets are running sums: entry e of the flat list lies at word e
    out[at] = flat[at]
    return out


CLASSES = ("zero", "one", "total_minus_1", "total", "mid", "boundary", "ample")
AMPLE_EXTRA = 37
# (U's class, Q's class): every class on either side, an overflow next to an ample list both ways round, the exact
# fit of both, NULL for both, and the full answer LAST -- into buffers that have seen every overflow before it
PAIRS = tuple((c, CLASSES[(i + 3) % len(CLASSES)]) for i, c in enumerate(CLASSES)) + (
    ("mid", "ample"), ("ample", "mid"), ("zero", "zero"), ("total", "total"), ("mid", "mid"), ("ample", "ample"))  # fmt: skip


def capacity_classes(counts: np.ndarray) -> dict:
    """Capacity per class for one list; a class the counts cannot give is left out."""
    counts = counts.astype(np.int64)
    total = int(counts.sum())
    off = np.cumsum(counts) - counts
    out = {"zero": 0, "one": 1, "total": total, "ample": total + AMPLE_EXTRA}
    if total >= 1:
        out["total_minus_1"] = total - 1
    half = total // 2
    inside = np.flatnonzero((counts >= 2) & (off >= 1) & (off + 1 >= half))  # one entry of the record fits, the next does not
    if inside.size:
        out["mid"] = int(off[inside[0]]) + 1
    ends = off + counts
    edge = np.flatnonzero((counts >= 1) & (ends > half // 2) & (ends < total) & (ends != out.get("mid", -1)))
    if edge.size:
        out["boundary"] = int(ends[edge[0]])
    return out


def capacity_pairs(ref: Reference) -> list:
    """[(U's class, Q's class, cap_u, cap_q)] of a case, in the order of PAIRS."""
    cu, cq = capacity_classes(ref.counts(0)), capacity_classes(ref.counts(1))
    return [(a, b, cu[a], cq[b]) for a, b in PAIRS if a in cu and b in cq]


# ---- window cases -----------------------------------------------------------------------------------

N_SITES = 3000
# records -> (sets, windows) in the wave form (1 to 3 sets) and in the shared form (4 to 20); a count with no such
# factorisation takes the nearest product above it (one record: 4 sets x 1 window)
COUNTS = {
    1: ((1, 1), (4, 1)),
    1023: ((3, 341), (11, 93)),
    1024: ((2, 512), (16, 64)),
    1025: ((1, 1025), (5, 205)),
    4096: ((2, 2048), (16, 256)),
    4097: ((1, 4097), (17, 241)),
    262144: ((2, 131072), (16, 16384)),
    262145: ((1, 262145), (13, 20165)),
    263168: ((2, 131584), (16, 16448)),  # 257 x 1024: the last grid in which every thread adds ONE partial
    263169: ((3, 87723), (9, 29241)),
    264020: ((2, 132010), (20, 13201)),
    265220: ((2, 132610), (20, 13261)),
}
GRIDS = {1: 1, 1023: 1, 1024: 1, 1025: 2, 4096: 4, 4097: 5, 262144: 256, 262145: 257, 263168: 257, 263169: 258, 264020: 258,
         265220: 260}  # fmt: skip
SECOND_PARTIAL_GRID = 258  # window_scan_apply: thread 0 of workgroup 257 is the first to add two partials
for _count, _forms in COUNTS.items():
    assert all(scan_grid(_s * _w) == GRIDS[_count] for _s, _w in _forms), _count


def _ranges(name: str, n_sites: int, n_windows: int):
    rng = _rng(name + "/windows")
    lo = rng.integers(0, n_sites - K + 1, n_windows).astype(np.int32)
    lo[-1] = n_sites - K  # the last window ends with the block
    lo[0] = 0
    return lo, lo + np.int32(K)


def _names():
    out = []
    for count, forms in COUNTS.items():
        for n_sets, n_w in forms:
            out.append(f"r{count}_{n_sets}x{n_w}")
    return out


SMALL_CLEAN, SMALL_MISSING = "small_clean_3x100", "small_missing_5x60"


@lru_cache(maxsize=None)
def window_case(name: str) -> WindowCase:
    if name in (SMALL_CLEAN, SMALL_MISSING):
        missing = name == SMALL_MISSING
        n_sets, n_w = (5, 60) if missing else (3, 100)
        blk = block("small missing" if missing else "small", 333, 0.06 if missing else 0.0)
        lo, hi = _ranges(name, 333, n_w)
        lo[1], lo[2] = 101, 104  # inside, and at the end of, the stretch without condition sites
        hi = lo + np.int32(K)
        start = 2 if missing else 3  # sets 2..6: both tight kinds and the one without ancestral alleles; 3..5 likewise
        return WindowCase(name, blk, [POOL[(start + j) % MAX_SETS] for j in range(n_sets)], lo, hi, large=not missing)
    count, dims = name[1:].split("_")
    n_sets, n_w = (int(v) for v in dims.split("x"))
    lo, hi = _ranges(name, N_SITES, n_w)
    start = _names().index(name)  # every case starts elsewhere in the pool: the tight sets meet the wave form too
    return WindowCase(name, block("large", N_SITES), [POOL[(start + j) % MAX_SETS] for j in range(n_sets)], lo, hi, large=True)


def window_case_names() -> list:
    return _names()


# ---- line cases ---------------------------------------------------------------------------------------

LINE_BLOCK = 4096  # text per workgroup of the count / scatter kernels; also how far the ninth tab is searched
LINE_SCAN_THREADS = 1024  # scan_blocks_kernel: one workgroup, ceil(n_blocks / 1024) blocks per thread
LINE_BLOCKS = (1024, 1025, 1536, 2048, 2049, 3001)
LINE_MIS = (0, 7)
HEAD_BYTES = 16


@lru_cache(maxsize=None)
def line_body() -> bytes:
    """VCF-shaped lines of 2 to 6 KB (a few empty and very short ones between them, so that some 4 KiB blocks hold
    several newlines and most hold none), longer than the largest case."""
    rng = _rng("lines")
    want = (max(LINE_BLOCKS) + 1) * LINE_BLOCK
    parts = [b"##meta\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\ts2\n"]
    size, i = len(parts[0]), 0
    while size < want:
        length = int(rng.integers(2048, 6145))
        fixed = b"21\t%d\t.\tA\tC\t.\tPASS\tDP=%d\tGT\t" % (i + 1, i % 90)
        line = fixed + (b"0|1\t" * (length // 4))[: length - len(fixed)]
        if i == 5:
            line = b"21\t6\t.\tA\tC\t.\tPASS\t" + b"X" * 4200 + b"\tGT\t0|1\t1|1"  # the ninth tab lies beyond 4 096 bytes
        elif i % 41 == 7:
            line = b"#" + line[1:]
        elif i % 41 == 13:
            line = b"21\t5\t" + b"s" * (length - 5)  # fewer than ten columns, longer than the search when length > 4 096
        elif i % 41 == 19:
            line = b"21\t5\tshort"
        elif i % 41 == 23:
            line = b""
        end = b"\r\n" if i % 5 == 2 else b"\n"
        parts.append(line + end)
        size += len(line) + len(end)
        i += 1
    return b"".join(parts)


def line_bytes(n_blocks: int, mis: int) -> int:
    """Text length for which the kernels use n_blocks blocks at base misalignment mis: the last block is full
    at misalignment 0 and holds a single byte otherwise."""
    return n_blocks * LINE_BLOCK if mis == 0 else (n_blocks - 1) * LINE_BLOCK + 1 - mis


def line_blocks(n_bytes: int, mis: int) -> int:
    return -(-(n_bytes + mis) // LINE_BLOCK)


@lru_cache(maxsize=None)
def _line_words():
    """(start of every line of the body, its fixed_len | cr << 31 word): per complete line the bytes up to and
    including the ninth tab, 1 for an empty or a '#' line, the line's length + 1 with fewer than ten columns, 4 097
    when the search of 4 096 bytes ends before either."""
    body = line_body()
    raw = np.frombuffer(body, dtype=np.uint8)
    ends = np.flatnonzero(raw == 10)
    starts = np.concatenate([[0], ends + 1]).astype(np.int64)
    words = np.zeros(len(ends), dtype=np.int64)
    for i in range(len(ends)):
        line = body[starts[i] : ends[i]]
        cr = line.endswith(b"\r")
        line = line[:-1] if cr else line
        fixed = 1
        if line and not line.startswith(b"#"):
            at = -1
            for _ in range(9):
                at = line.find(b"\t", at + 1, LINE_BLOCK)
                if at < 0:
                    break
            fixed = at + 1 if at >= 0 else (len(line) + 1 if len(line) <= LINE_BLOCK else LINE_BLOCK + 1)
        words[i] = fixed | ((1 << 31) if cr else 0)
    return starts, words


@dataclass
class LineCase:
    n_blocks: int
    mis: int
    text: bytes
    starts: np.ndarray  # int64 [n_lines + 1]: 0 and the byte behind every newline
    words: np.ndarray  # int64 [n_lines]

    @property
    def n_lines(self) -> int:
        return int(self.words.size)

    def heads(self, head_bytes: int = HEAD_BYTES) -> np.ndarray:
        """uint8 [n_lines][head_bytes]: the first bytes of every line, its newline included, padded with newlines."""
        raw = np.frombuffer(self.text, dtype=np.uint8)
        at = self.starts[:-1, None] + np.arange(head_bytes)[None, :]
        inside = at < self.starts[1:, None]
        return np.where(inside, raw[np.minimum(at, raw.size - 1)], 10).astype(np.uint8)


@lru_cache(maxsize=None)
def line_case(n_blocks: int, mis: int) -> LineCase:
    text = line_body()[: line_bytes(n_blocks, mis)]
    raw = np.frombuffer(text, dtype=np.uint8)
    starts = np.concatenate([[0], np.flatnonzero(raw == 10) + 1]).astype(np.int64)
    all_starts, all_words = _line_words()
    n_l = starts.size - 1
    assert np.array_equal(starts, all_starts[: n_l + 1])
    return LineCase(n_blocks, mis, text, starts, all_words[:n_l])
