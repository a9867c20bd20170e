"""The cases of the direct tests of ``sai_tokenize_gt`` (test_tokenize_cases_cpu.py, test_tokenize_device.py): text
buffers with a line table built by hand, and what every line must give -- from a statement of the genotype rules
written here from their wording (DESIGN_INGEST.md, "GPU: tokenise"), not from either C++ loop.

A case is one launch: ``text`` (bytes, a multiple of 4 long), the line table (``off`` int64, ``len`` int32, ``flip`` and
``gi`` uint8), ``n_cols``, ``slot_of_col``, ``n_out``, ``ploidy``, and the statement's ``rows`` (int8 [lines][n_out],
``SENTINEL`` in the slots no column maps to), ``status`` (0 / 1) and ``why`` (the host reader's wording for a refused
line).  ``kind`` groups the cases; ``host`` is False where the host reader cannot be asked (a ploidy above its limit
of 64).  Every byte of ``text`` outside the lines is a tab or a digit, the byte before a line that does not follow
another line directly is a tab, and so is the byte behind the last line of a buffer: a kernel that looks one byte too
far sees another line.

The kernel walks a line in steps of 256 bytes from ``c0 = off & ~3``, lane ``l`` holding bytes ``4 l .. 4 l + 3`` of
the step; ``position(off, p)`` names the (step, lane, byte) of a text offset by that arithmetic alone."""

import functools
import re
from types import SimpleNamespace

import numpy as np

MAX_ALLELE = 100000  # SAI_GT_MAX_ALLELE of include/saihip.h (test_tokenize_cases_cpu.py compares them)
SENTINEL = 85
STEP = 256
UNPARSABLE, TOO_FEW, RANGE = "unparsable genotype", "too few sample columns", "int8"

# ---- the statement ----------------------------------------------------------------------------------------------

# an allele: '.', a run of digits, or nothing where a separator, ':' or the end of the field comes next
_ALLELE = re.compile(rb"\.|[0-9]+|(?=[|/:]|$)")


@functools.lru_cache(maxsize=None)
def field_result(field: bytes, gi: int, pl: int):
    """(d, fd, None) of one sample field cut at the tabs, or (None, None, the host reader's reason) where it is refused."""
    at = 0
    for _ in range(gi):  # a skip runs to the next ':' and passes it; at the end of the field it stays there
        colon = field.find(b":", at)
        at = len(field) if colon < 0 else colon + 1
    alleles = []
    while True:
        m = _ALLELE.match(field, at)
        if m is None:
            return None, None, UNPARSABLE
        word, at = m.group(), m.end()
        if word.isdigit() and int(word) > MAX_ALLELE:
            return None, None, RANGE  # wherever it stands, counted or not
        alleles.append(int(word) if word.isdigit() else -1)
        if field[at : at + 1] in (b"|", b"/"):
            at += 1
        else:
            break  # the first character behind an allele that is no separator ends the reading
    counted = (alleles + [-1] * pl)[:pl]
    d = sum(counted)
    fd = sum(a - 1 if a >= 1 else 1 - a for a in counted)
    if d > 127 or fd > 127 or d < -128:
        return None, None, RANGE
    return d, fd, None


def gt_field(field: bytes, gi: int, pl: int):
    """(d, fd) of one sample field, or None where the rules refuse it."""
    d, fd, why = field_result(bytes(field), gi, pl)
    return None if why else (d, fd)


def line_row(section: bytes, gi: int, flip: int, slot_of_col, ploidy_of_slot, n_out: int):
    """(row int8 [n_out], status, why) of one line's sample section.  The columns are taken in order, as the host
    reader names the first thing it meets."""
    fields = bytes(section).split(b"\t")  # b"" -> one empty field; a trailing tab -> one more empty field
    row = np.full(n_out, SENTINEL, dtype=np.int8)
    for col, slot in enumerate(slot_of_col):
        if col >= len(fields):
            return row, 1, TOO_FEW
        if slot < 0:
            continue
        d, fd, why = field_result(fields[col], int(gi), int(ploidy_of_slot[slot]))
        if why:
            return row, 1, why
        row[slot] = fd if flip else d
    return row, 0, None


# ---- the layout of a buffer ---------------------------------------------------------------------------------------


def position(off: int, p: int):
    """(step, lane, byte of the lane's word) of text offset ``p`` in the walk of the line that starts at ``off``."""
    rel = p - (off & ~3)
    return rel // STEP, rel % STEP // 4, rel % 4


def start_class(off: int, p: int) -> str:
    """How the kernel learns that a field starts at ``p``: which byte holds the tab before it."""
    step, lane, k = position(off, p)
    if p == off:
        return "first"
    if k > 0:
        return "own"
    return "below" if lane > 0 else "carry"


class Layout:
    """A text buffer under construction and its line table."""

    def __init__(self):
        self.buf, self.lines = bytearray(), []

    def gap(self, mod: int) -> None:
        """One to four bytes of poison -- a tab, digits, a tab -- so that the next byte lies at ``mod`` (mod 4)."""
        n = (mod - len(self.buf)) % 4 or 4
        self.buf += (b"\t", b"\t\t", b"\t1\t", b"\t12\t")[n - 1]

    def add(self, section: bytes, mod=None, flip: int = 0, gi: int = 0, **tag) -> None:
        """A line; ``mod`` = its offset mod 4 behind a gap, None = directly behind the line before it."""
        if mod is not None:
            self.gap(mod)
        self.lines.append(SimpleNamespace(off=len(self.buf), len=len(section), flip=flip, gi=gi, **tag))
        self.buf += section

    def close(self, slack=None) -> bytes:
        """The buffer, a multiple of 4 long: ``slack`` poison bytes behind the last line (it must come out even), or
        one to four."""
        if slack is None:
            self.gap(0)
        else:
            self.buf += b"\t56"[:slack]
            assert len(self.buf) % 4 == 0, (len(self.buf), slack)
        return bytes(self.buf)


def make_case(name, kind, layout, slot_of_col, n_out, ploidy, slack=None, host=True, **meta):
    text = layout.close(slack)
    lines = layout.lines
    slot_of_col = np.asarray(slot_of_col, dtype=np.int32)
    ploidy = np.asarray(ploidy, dtype=np.int32)
    rows = np.empty((len(lines), n_out), dtype=np.int8)
    status = np.empty(len(lines), dtype=np.int32)
    why = []
    slots, pl = slot_of_col.tolist(), ploidy.tolist()
    for i, ln in enumerate(lines):
        rows[i], status[i], reason = line_row(text[ln.off : ln.off + ln.len], ln.gi, ln.flip, slots, pl, n_out)
        why.append(reason)
    return SimpleNamespace(name=name, kind=kind, text=text, lines=lines, n_lines=len(lines),
                           off=np.array([ln.off for ln in lines], dtype=np.int64), len=np.array([ln.len for ln in lines], dtype=np.int32),
                           flip=np.array([ln.flip for ln in lines], dtype=np.uint8), gi=np.array([ln.gi for ln in lines], dtype=np.uint8),
                           n_cols=len(slot_of_col), slot_of_col=slot_of_col, n_out=int(n_out), ploidy=ploidy, rows=rows, status=status,
                           why=why, host=host, meta=SimpleNamespace(**meta))  # fmt: skip


def check_contract(case) -> None:
    """What ``sai_tokenize_gt`` asks of its caller, and what the cases promise about the bytes around the lines.
    A table that points outside the buffer would fault the GPU: this runs before every launch."""
    text, n = case.text, len(case.text)
    assert n % 4 == 0 and n > 0
    assert case.off.dtype == np.int64 and case.len.dtype == np.int32 and case.flip.dtype == np.uint8 and case.gi.dtype == np.uint8
    assert case.slot_of_col.dtype == np.int32 and case.ploidy.dtype == np.int32
    assert len(case.off) == len(case.len) == len(case.flip) == len(case.gi) == case.n_lines >= 1
    assert (case.off >= 0).all() and (case.len >= 0).all() and (case.off + case.len <= n).all()
    assert case.n_out >= 1 and len(case.ploidy) == case.n_out and (case.ploidy >= 1).all()
    assert len(case.slot_of_col) == case.n_cols >= 1
    mapped = case.slot_of_col[case.slot_of_col >= 0]
    assert (case.slot_of_col >= -1).all() and (mapped < case.n_out).all() and len(set(mapped.tolist())) == len(mapped)
    assert case.slot_of_col[-1] >= 0  # the host reader's column count ends at the last selected column
    assert case.rows.shape == (case.n_lines, case.n_out) and case.rows.dtype == np.int8 and set(case.status.tolist()) <= {0, 1}
    inside = np.zeros(n + 1, dtype=np.int32)
    np.add.at(inside, case.off, 1)
    np.add.at(inside, case.off + case.len, -1)
    inside = np.cumsum(inside)[:n]
    assert inside.max() <= 1  # no two lines share a byte
    raw = np.frombuffer(text, dtype=np.uint8)
    outside = raw[inside == 0]
    assert np.isin(outside, np.frombuffer(b"\t0123456789", dtype=np.uint8)).all()
    ends, offs = set((case.off + case.len).tolist()), set(case.off.tolist())
    for i in range(case.n_lines):
        off, end = int(case.off[i]), int(case.off[i] + case.len[i])
        assert b"\n" not in text[off:end] and b"\r" not in text[off:end]
        if off not in ends or case.len[i] == 0:  # not directly behind another line
            assert off > 0 and text[off - 1 : off] == b"\t"
        if end < n and end not in offs:
            assert text[end : end + 1] == b"\t"


# ---- the start-position sweep ---------------------------------------------------------------------------------------

SWEEP_T = 3 * STEP + 8  # a selected field starts at off + t for every t in 0 .. SWEEP_T
SHAPES = (b"0|1", b".", b"", b"10|2:7")
SWEEP_COLS = SWEEP_T // 2 + 4  # the run of two-byte fields brings the swept field to column t / 2


def junk(n: int) -> bytes:
    """``n`` bytes without a tab that read as the allele 0 at gi = 0 and hold anything behind the first ':'."""
    return (b"0:" + b"x|/.:9-" * (n // 7 + 1))[:n]


def digit_of(col: int) -> bytes:
    return b"%d" % (col % 7)  # neighbouring columns differ, so a column number that is off by a few shows


def sweep_line(t: int, prefix: str, pick: int) -> bytes:
    """A line whose field ``SHAPES[pick % 4]`` starts at byte ``t``.  ``junk``: one field of t - 1 bytes and a tab in
    front of it (the field is column 1; column 0 at t = 0).  ``run``: fields of one digit and a tab in front of it, one
    empty field first where t is odd (column about t / 2).  ``SHAPES[(pick + 1) % 4]`` follows, then empty fields up to
    ``SWEEP_COLS`` columns, the last one a digit."""
    if prefix == "junk":
        head = [junk(t - 1)] if t else []
    else:
        head = ([b""] if t % 2 else []) + [digit_of(c + t % 2) for c in range(t // 2)]
    fields = head + [SHAPES[pick % 4], SHAPES[(pick + 1) % 4]]
    fields += [b""] * (SWEEP_COLS - len(fields) - 1) + [digit_of(SWEEP_COLS - 1)]
    line = b"\t".join(fields)
    assert len(fields) == SWEEP_COLS and (line[t - 1 : t] == b"\t" or t == 0) and len(b"\t".join(head)) + bool(head) == t
    return line


@functools.lru_cache(maxsize=None)
def sweep_case():
    """Every t x every off % 4 x both prefixes in ONE launch: every column is selected, through a permutation, and two
    slots of the row belong to no column."""
    rng = np.random.default_rng(20261021)
    lay = Layout()
    for prefix in ("junk", "run"):
        for mod in range(4):
            for t in range(SWEEP_T + 1):
                lay.add(sweep_line(t, prefix, t + mod + (prefix == "run")), mod, swept=t, prefix=prefix, offmod=mod)
    n_out = SWEEP_COLS + 2
    slots = rng.permutation(n_out)[:SWEEP_COLS]
    ploidy = [(1, 2, 2, 3)[s % 4] for s in range(n_out)]
    return make_case("sweep", "sweep", lay, slots, n_out, ploidy)


def field_starts(case, i):
    """The text offsets at which the fields of line ``i`` start, by column."""
    off, n = int(case.off[i]), int(case.len[i])
    section = case.text[off : off + n]
    return [off] + [off + k + 1 for k in range(n) if section[k] == 9]


# ---- line ends ------------------------------------------------------------------------------------------------------

END_RESIDUES = (0, 1, 2, 255)


@functools.lru_cache(maxsize=None)
def line_end_case():
    """Lines of four columns, all selected, that end at ``(end - c0) % 256`` in END_RESIDUES after one, two or three
    steps, the last field ``0|1`` or -- behind a trailing tab -- empty.  A trailing tab at residue 0 is lane 63 byte 3
    of its step."""
    lay = Layout()
    for steps in (1, 2, 3):
        for residue in END_RESIDUES:
            for mod in range(4):
                for trailing in (False, True):
                    span = STEP * (steps - 1) + (residue or STEP)  # end - c0
                    tail = b"\t1|1\t.\t" + (b"" if trailing else b"0|1")
                    fill = span - mod - len(tail)
                    if fill < 0:
                        continue  # a line of one or two bytes at off % 4 = 3 has no room for four columns
                    lay.add(junk(fill) + tail, mod, flip=(steps + mod) % 2, residue=residue, trailing=trailing, steps=steps)
    return make_case("line_ends", "line_end", lay, [2, 0, 3, 1], 5, [2, 2, 1, 2, 2])


@functools.lru_cache(maxsize=None)
def empty_line_cases():
    """``len == 0`` at every off % 4: one missing call with one column, flagged with two."""
    out = []
    for n_cols in (1, 2):
        lay = Layout()
        for mod in range(4):
            lay.add(b"", mod, flip=mod % 2)
        out.append(make_case(f"empty_{n_cols}col", "rules", lay, list(range(n_cols)), n_cols, [2] * n_cols))
    return out


# ---- a long line ----------------------------------------------------------------------------------------------------

LONG_FIELDS = 5000


def long_fields(rng, spoil=()):
    """``LONG_FIELDS`` fields ``DP:GT[:more]`` (gi = 1) of one to four alleles, some of several digits, some missing,
    some fields cut short before their GT; the columns of ``spoil`` hold what no reader may parse."""
    fields = []
    for c in range(LONG_FIELDS):
        n = int(rng.integers(1, 5))
        alleles = [str(rng.choice([".", "0", "1", "2", "10", "11", ""], p=[0.1, 0.35, 0.3, 0.1, 0.05, 0.05, 0.05])) for _ in range(n)]
        gt = "".join(a + str(rng.choice(["|", "/"])) for a in alleles)[:-1]
        kind = int(rng.integers(8))
        text = f"{int(rng.integers(0, 200))}:{gt}" + (f":{int(rng.integers(0, 99))}:x,y" if kind < 3 else "")
        if kind == 7:
            text = str(int(rng.integers(0, 50)))  # no GT sub-field at all: a missing call
        fields.append(b"0|x:&:7" if c in spoil else text.encode())
    return fields


@functools.lru_cache(maxsize=None)
def long_line_cases():
    """(every column selected through a permutation; every 97th column selected, more slots than columns mapped)"""
    rng = np.random.default_rng(97)
    lay = Layout()
    lay.add(b"\t".join(long_fields(rng)), 1, flip=0, gi=1)
    lay.add(b"\t".join(long_fields(rng)), 3, flip=1, gi=1)
    n_out = LONG_FIELDS + 3
    slots = rng.permutation(n_out)[:LONG_FIELDS]
    every = make_case("long_all_columns", "long", lay, slots, n_out, [(2, 1, 4, 3, 2)[s % 5] for s in range(n_out)])
    n_cols = 97 * 51 + 1  # the last column of the count is a selected one; 52 fields follow it
    picked = set(range(0, n_cols, 97))
    lay = Layout()
    lay.add(b"\t".join(long_fields(rng, spoil=set(range(LONG_FIELDS)) - picked)), 2, flip=0, gi=1)
    lay.add(b"\t".join(long_fields(rng, spoil=set(range(LONG_FIELDS)) - picked)), 0, flip=1, gi=1)
    sparse_slots = np.full(n_cols, -1, dtype=np.int32)
    sparse_slots[sorted(picked)] = rng.permutation(70)[: len(picked)]
    sparse = make_case("long_every_97th", "long", lay, sparse_slots, 70, [(2, 1, 4, 3, 2)[s % 5] for s in range(70)])
    return [every, sparse]


# ---- fields and digit runs across a step boundary -------------------------------------------------------------------

STRADDLE = b"12|345:99"


@functools.lru_cache(maxsize=None)
def straddle_case():
    """The first and the second step boundary at every byte of ``12|345:99`` (and just before and behind it), at every
    off % 4.  gi = 0 reads 12 at ploidy 1 (345 is read and dropped), gi = 1 skips across the boundary and reads 99.  The
    field in front is not selected: at gi = 1 it could not be parsed."""
    lay = Layout()
    for boundary in (STEP, 2 * STEP):
        for mod in range(4):
            for j in range(len(STRADDLE) + 1):  # the boundary lies before byte j of the field
                t = boundary - mod - j
                for gi in (0, 1):
                    lay.add(junk(t - 1) + b"\t" + STRADDLE + b"\t7|8", mod, flip=(j + gi) % 2, gi=gi, boundary=boundary, at=j, swept=t)
    return make_case("straddle", "straddle", lay, [-1, 3, 0], 4, [2, 1, 2, 1])


# ---- the rules, one line each ---------------------------------------------------------------------------------------


def _table(name, entries, slot_of_col, n_out, ploidy, host=True):
    lay = Layout()
    for k, (section, gi, flip, note) in enumerate(entries):
        lay.add(section, k % 4, flip=flip, gi=gi, note=note)
    return make_case(name, "rules", lay, slot_of_col, n_out, ploidy, host=host)


@functools.lru_cache(maxsize=None)
def rules_cases():
    """Columns 0, 2, 3, 4 are read at ploidy 1, 2, 3, 4, column 5 at ploidy 2 again; column 1 is not selected; slot 4
    belongs to no column.  Every refused line stands behind an accepted one that differs from it by one value."""
    slot_of_col, n_out, ploidy = [3, -1, 0, 5, 2, 1], 6, [2, 2, 4, 1, 7, 3]

    def same(field, gi=0, flip=0, note="", unselected=b"0|1"):
        cols = [field, unselected, field, field, field, field]
        return b"\t".join(cols), gi, flip, note

    def one(field, gi=0, flip=0, note="", col=2, other=b"0|1"):
        cols = [other] * 6
        cols[col] = field
        return b"\t".join(cols), gi, flip, note

    entries = []
    for flip in (0, 1):
        entries += [
            same(b"1|1|1|1", 0, flip, "cut to the ploidy"),
            same(b"1", 0, flip, "padded with missing alleles"),
            same(b"2/0|.", 0, flip, "both separators, a missing allele"),
            same(b"", 0, flip, "an empty field"),
            same(b".", 0, flip, "a lone dot"),
            same(b"|1", 0, flip, "an empty first allele"),
            same(b"1|", 0, flip, "an empty last allele"),
            same(b"/", 0, flip, "two empty alleles"),
            same(b".5|1", 0, flip, "a dot, then something that is no separator: the reading stops"),
            same(b"0x", 0, flip, "0x reads as the single allele 0"),
            same(b"1x|1", 0, flip, "what follows the stop is never read"),
            same(b"0000000000001|010", 0, flip, "leading zeros are no large value"),
            same(b"1|1:9|9:x", 0, flip, "sub-fields behind GT"),
            same(b"7:1|0", 1, flip, "gi = 1"),
            same(b"7", 1, flip, "gi = 1, the field ends before GT"),
            same(b"7:", 1, flip, "gi = 1, GT is there and empty"),
            same(b"x|y:1/1:z", 1, flip, "gi = 1, anything in the sub-field before GT"),
            same(b"1:2:3:1|1|0", 3, flip, "gi = 3"),
            same(b"1:2", 3, flip, "gi = 3, two sub-fields only"),
            same(b"1:2:3", 3, flip, "gi = 3, the field ends before GT"),
            same(b"1:2:3::1", 3, flip, "gi = 3, an empty GT and more behind it"),
            same(b"", 3, flip, "gi = 3, an empty field"),
            one(b"0|1|9|9|9", 0, flip, "alleles beyond the ploidy"),
            one(b"63|64", 0, flip, "d = 127 is kept"),
            one(b"64|64", 0, flip, "d = 128 is refused"),
            one(b"0|1|100000", 0, flip, "the largest allele index, beyond the ploidy"),
            one(b"0|1|100001", 0, flip, "one more is refused, counted or not"),
            one(b"0|99999999999", 0, flip, "eleven digits: refused before they wrap"),
            one(b"0|99999999999", 0, flip, "the same in the column that is not selected", col=1),
            one(b"0|1|100001", 0, flip, "the same in the column that is not selected", col=1),
            one(b"0|x", 0, flip, "unparsable in a selected column"),
            one(b"0|x", 0, flip, "the same in the column that is not selected", col=1),
            one(b"0|1|x", 0, flip, "unparsable beyond the ploidy"),
            one(b"0|1|", 0, flip, "an empty allele beyond the ploidy"),
            one(b"2|1\t0|x\tx\t\t&", 0, flip, "more fields than columns: the extra ones are never read", col=5),
            (b"\t".join([b"0|1"] * 6), 0, flip, "exactly the columns asked for"),
            (b"\t".join([b"0|1"] * 5), 0, flip, "one column short"),
            (b"\t".join([b"0|1"] * 5) + b"\t", 0, flip, "a trailing tab opens the last column"),
            (b"\t" * 5, 0, flip, "six empty fields"),
            (b"\t" * 4, 0, flip, "five empty fields"),
        ]
    out = [_table("rules", entries, slot_of_col, n_out, ploidy)]
    # the other edge of the range: a missing allele counts 2 towards fd, so 63 of them are kept (fd = 126) and 64 are
    # not (fd = 128) -- on a flipped line or not, since a field is refused whichever of d and fd the line uses.  d < -128
    # cannot be met without fd > 127.
    mixed = lambda n: b"|".join([b"1", b"0"] * (n // 2) + [b"1"] * (n % 2))  # noqa: E731  d = ceil(n / 2), fd = floor(n / 2)
    edge = []
    for flip in (0, 1):
        edge += [((mixed(63) + b"\t" + mixed(64)), 0, flip, "63 and 64 alleles within the range"),
                 ((b".\t" + mixed(64)), 0, flip, "ploidy 63, all missing: d = -63, fd = 126"),
                 ((mixed(63) + b"\t."), 0, flip, "ploidy 64, all missing: fd = 128"),
                 ((mixed(63) + b"\t" + b"|".join([b"1"] * 64)), 0, flip, "ploidy 64, all 1: d = 64, fd = 0"),
                 ((mixed(63) + b"\t" + b"|".join([b"2"] * 64)), 0, flip, "ploidy 64, all 2: d = 128")]  # fmt: skip
    out.append(_table("rules_ploidy_63_64", edge, [0, 1], 2, [63, 64]))
    high = []
    for flip in (0, 1):
        high += [((mixed(128) + b"\t" + mixed(129)), 0, flip, "128 and 129 alleles within the range"),
                 ((b".\t" + mixed(129)), 0, flip, "ploidy 128, all missing: d = -128 but fd = 256"),
                 ((mixed(128) + b"\t."), 0, flip, "ploidy 129, all missing: d = -129"),
                 ((mixed(127) + b"\t" + mixed(129)), 0, flip, "ploidy 128, one allele short: d = 63, fd = 65"),
                 ((mixed(128) + b"|1\t" + mixed(129) + b"|1"), 0, flip, "one more allele than the ploidy")]  # fmt: skip
    out.append(_table("rules_ploidy_128_129", high, [0, 1], 2, [128, 129], host=False))  # the host reader takes ploidies up to 64
    return out + empty_line_cases()


# ---- the launch shape -----------------------------------------------------------------------------------------------

LAUNCH_LINES = (1, 3, 4, 5, 9)  # the kernel takes four lines per workgroup


@functools.lru_cache(maxsize=None)
def launch_cases():
    """``n`` lines back to back, the last one ending 0 .. 3 bytes before the end of the buffer.  The last line is 4 k + 2
    bytes long and ends in a tab and one digit, so its last tab shares a word with the end of the buffer whatever the
    alignment the words are read at."""
    out = []
    for n in LAUNCH_LINES:
        for slack in range(4):
            sections = [b"%d|1\t%d\t.|%d" % (i % 3, (i + slack) % 10, i % 2) + b":7" * (i % 3) for i in range(n - 1)]
            sections.append(b"1|0\t1%d|1\t%d" % (n % 2, slack))
            assert len(sections[-1]) % 4 == 2
            total = sum(len(s) for s in sections)
            lay = Layout()
            lay.gap((-slack - total) % 4)
            for i, s in enumerate(sections):
                lay.add(s, None, flip=i % 2)
            out.append(make_case(f"launch_{n}_lines_slack_{slack}", "launch", lay, [1, 0, 3], 4, [2, 1, 2, 2], slack=slack, slack_bytes=slack))
    return out


def all_cases():
    return [sweep_case(), line_end_case(), *long_line_cases(), straddle_case(), *rules_cases(), *launch_cases()]
