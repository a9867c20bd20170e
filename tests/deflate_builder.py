"""A test-side DEFLATE (RFC 1951) *encoder* that takes its decisions from the caller or from a seeded
RNG instead of making them well: the block kinds, the parse into literals and matches, the Huffman
code lengths (random complete prefix codes, chains of up to 15 bits), the run-length coding of the
code lengths and the padding of the header counts are all chosen, not optimised.  It reaches the
parts of the format that zlib's own encoder never emits, and it keeps the expected text by applying
the tokens itself, so every stream has two independent statements of its text: this module's and
zlib's decoder (tests/test_deflate_builder_cpu.py proves them equal before a kernel is judged).

No tests in here; pure Python with zlib and numpy only."""

import bisect
import struct
import zlib

import numpy as np

WINDOWS = (4096, 8192, 16384, 32768)  # the history sizes sai_inflate_bgzf is instantiated for

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]  # fmt: skip
DIST_EXTRA = [0, 0, 0, 0] + [x for x in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST_LENS = [5] * 32


class BitWriter:
    """LSB-first fields, MSB-first Huffman codes (RFC 1951 3.1.1)."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, n):
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.n
        self.n += n
        if self.n >= 512:
            self._flush_whole()

    def code(self, code, n):
        self.bits(reverse_bits(code, n), n)

    def align(self):
        self.bits(0, -self.pos % 8)

    def _flush_whole(self):
        k = self.n >> 3
        if k:
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def raw(self, data):
        assert self.pos % 8 == 0
        self._flush_whole()
        self.out += data

    @property
    def pos(self):
        return 8 * len(self.out) + self.n

    def getvalue(self):
        """The bytes so far (a last partial byte filled with zero bits); the writer stays usable."""
        self._flush_whole()
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def reverse_bits(code, n):
    return int(format(code, "0%db" % n)[::-1], 2) if n else 0


def patch_bits(raw, pos, n, value):
    """`raw` with the n-bit LSB-first field at bit `pos` replaced by `value`."""
    x = int.from_bytes(raw, "little")
    x = (x & ~(((1 << n) - 1) << pos)) | (value << pos)
    return x.to_bytes(len(raw), "little")


def length_symbol(length, alt258=False):
    """(symbol, extra bits, extra value) of a match length; 258 either as 285 or as 284 + 31."""
    if length == 258 and not alt258:
        return 285, 0, 0
    i = bisect.bisect_right(LEN_BASE, length, 0, 28) - 1
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def distance_symbol(dist):
    i = bisect.bisect_right(DIST_BASE, dist) - 1
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


def canonical_codes(lens):
    """The canonical code of every symbol (RFC 1951 3.2.2); also defined, if meaningless, for an
    over-subscribed set."""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    codes = [0] * len(lens)
    for s, n in enumerate(lens):
        if n:
            codes[s] = nxt[n] & ((1 << n) - 1)
            nxt[n] += 1
    return codes


def kraft(lens):
    """Sum of 2^-len in units of 2^-15: 32768 for a complete code."""
    return sum(1 << (15 - n) for n in lens if n)


def random_prefix_depths(rng, n, max_depth, skew):
    """The depths of the n leaves of a random full binary tree: start from one leaf and split leaves
    until there are n.  `skew` is the chance of splitting the deepest leaf that may still be split,
    which gives chain codes up to `max_depth` bits.  The Kraft sum is exactly 1 (n >= 2)."""
    assert 1 <= n <= (1 << max_depth)
    if n == 1:
        return [1]  # a single code of one bit: incomplete, legal for the two block alphabets
    leaves = [0]
    while len(leaves) < n:
        open_ = [i for i, d in enumerate(leaves) if d < max_depth]
        if rng.random() < skew:
            top = max(leaves[i] for i in open_)
            i = next(i for i in open_ if leaves[i] == top)
        else:
            i = open_[int(rng.integers(len(open_)))]
        leaves[i] += 1
        leaves.append(leaves[i])
    return leaves


def random_code_lengths(rng, used, n_symbols, max_depth, skew, extra=0.0, deep=()):
    """Code lengths for an alphabet of `n_symbols`: a random complete prefix code over the `used`
    symbols plus (chance `extra`) a few random symbols from outside them, the leaves dealt to the
    symbols at random; the symbols in `deep` are then handed the deepest leaves."""
    syms = set(used)
    if extra and rng.random() < extra:
        for s in rng.integers(0, n_symbols, size=int(rng.integers(1, 12))):
            syms.add(int(s))
    syms = sorted(syms)
    depths = random_prefix_depths(rng, len(syms), max_depth, skew)
    order = rng.permutation(len(syms))
    lens = [0] * n_symbols
    for k, d in zip(order, depths):
        lens[syms[int(k)]] = d
    for s in deep:
        top = max(range(n_symbols), key=lambda t: lens[t])
        lens[s], lens[top] = lens[top], lens[s]
    return lens


def rle_random(rng, lens):
    """The code-length sequence (symbol, extra value) of `lens`, each step chosen at random among the
    legal alternatives: the length itself, 16 (repeat the previous length 3-6 times), 17 / 18 (3-10 /
    11-138 zeros), with random run splits.  `lens` is the literal/length lengths followed by the
    distance lengths, so runs cross that boundary freely."""
    seq, i, n = [], 0, len(lens)
    while i < n:
        v = lens[i]
        run = 1
        while i + run < n and lens[i + run] == v:
            run += 1
        opts = ["lit"]
        if v == 0 and run >= 3:
            opts.append(17)
        if v == 0 and run >= 11:
            opts += [18, 18]
        if i > 0 and lens[i - 1] == v and run >= 3:
            opts += [16, 16]
        o = opts[int(rng.integers(len(opts)))]
        if o == "lit":
            seq.append((v, 0))
            i += 1
        else:
            lo, hi = {16: (3, 6), 17: (3, 10), 18: (11, 138)}[o]
            rep = int(rng.integers(lo, min(hi, run) + 1))
            seq.append((o, rep - lo))
            i += rep
    return seq


def expand_cl_seq(seq, total=None):
    """The code lengths a code-length sequence stands for (a leading 16 repeats 0, as this module
    needs a definite code to go on writing an invalid stream); cut at `total`."""
    lens = []
    for sym, extra in seq:
        if sym < 16:
            lens.append(sym)
        elif sym == 16:
            lens += [lens[-1] if lens else 0] * (3 + extra)
        else:
            lens += [0] * ((3 if sym == 17 else 11) + extra)
    return lens if total is None else lens[:total]


def new_stats():
    return {
        "blocks": {"stored": 0, "fixed": 0, "dynamic": 0},
        "maxcode": {"lit": 0, "len": 0, "eob": 0, "dist": 0},  # the longest code actually emitted
        "wclass": {(w, o): 0 for w in WINDOWS for o in (-1, 0, 1)},  # matches at distance W + o
        "overlap": 0,  # matches that read their own output
        "first_match": 0,  # a match as the first symbol of a block
        "stored_bit_offset": [0] * 8,  # where in its byte a stored block's header starts
        "alt258": 0,
        "rep16_cross": 0,  # a 16 that runs from the literal/length lengths into the distance lengths
        "rep16_after16": 0,
        "rep16_after_zeros": 0,  # a 16 right after a 17 or an 18
        "single_dist_code": 0,
        "n_lit": set(),
        "n_dist": set(),
        "n_cl": set(),
    }


class Member:
    """One raw DEFLATE stream under construction: block writers that take tokens -- ('L', byte),
    ('M', length, distance[, alt258]) -- or raw bytes, the text they stand for, the feature counters,
    and the bit positions of the header fields (`marks`) for the writers of invalid streams.
    Tokens for invalid streams only: ('S', symbol) / ('D', symbol) write the bare code of a
    literal/length / distance symbol; after one of them, or after a match that reaches back beyond
    the text, the text is no longer tracked."""

    def __init__(self):
        self.w = BitWriter()
        self.text = bytearray()
        self.stats = new_stats()
        self.marks = []  # one dict per block
        self.broken = False

    # ---- blocks ----
    def _header(self, final, btype, kind):
        self.marks.append({"kind": kind, "start": self.w.pos, "btype": self.w.pos + 1})
        self.stats["blocks"][kind] += 1
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)

    def stored(self, data, final=False):
        assert len(data) <= 65535
        self.stats["stored_bit_offset"][self.w.pos % 8] += 1
        self._header(final, 0, "stored")
        self.w.align()
        self.marks[-1]["len"] = self.w.pos
        self.marks[-1]["nlen"] = self.w.pos + 16
        self.w.bits(len(data), 16)
        self.w.bits(len(data) ^ 0xFFFF, 16)
        self.w.raw(bytes(data))
        self.text += data
        return self

    def fixed(self, tokens, final=False, emit_eob=True):
        self._header(final, 1, "fixed")
        self._body(tokens, FIXED_LIT_LENS, FIXED_DIST_LENS, emit_eob)
        return self

    def dynamic(self, tokens, final=False, rng=None, skew=0.0, extra=0.3, pad=True, deep_eob=0.0, lit_lens=None, dist_lens=None,
                cl_seq=None, n_lit=None, n_dist=None, n_cl=None, cl_lens=None, emit_eob=True, check=True):  # fmt: skip
        """A dynamic block.  By default everything is drawn from `rng`; `lit_lens` / `dist_lens` fix the
        two codes, `cl_seq` fixes the code-length sequence (and with it both codes), `n_lit` / `n_dist`
        / `n_cl` fix the header counts, `cl_lens` the code-length code.  `check=False` lets a stream
        that is invalid on purpose through."""
        rng = rng if rng is not None else np.random.default_rng(0)
        if cl_seq is not None:
            lens = expand_cl_seq(cl_seq, n_lit + n_dist)
            lens += [0] * (n_lit + n_dist - len(lens))
            lit_lens, dist_lens = lens[:n_lit], lens[n_lit:]
        else:
            used_lit, used_dist = {256}, set()
            for t in tokens:
                if t[0] == "L":
                    used_lit.add(t[1])
                elif t[0] == "M":
                    used_lit.add(length_symbol(t[1], len(t) > 3 and t[3])[0])
                    used_dist.add(distance_symbol(t[2])[0])
            if lit_lens is None:
                if len(used_lit) == 1:
                    used_lit.add(int(rng.integers(0, 256)))  # zlib wants the literal/length code complete
                deep = [256] if rng.random() < deep_eob else []
                lit_lens = random_code_lengths(rng, used_lit, 286, 15, skew, extra, deep)
            if dist_lens is None:
                dist_lens = random_code_lengths(rng, used_dist, 30, 15, skew, extra) if used_dist else [0] * 30
            lit_lens, dist_lens = list(lit_lens), list(dist_lens)
            min_lit = max(257, max(i for i, n in enumerate(lit_lens) if n) + 1) if any(lit_lens) else 257
            min_dist = max([1] + [i + 1 for i, n in enumerate(dist_lens) if n])
            if n_lit is None:
                n_lit = int(rng.integers(min_lit, 287)) if pad and rng.random() < 0.5 else min_lit
            if n_dist is None:
                n_dist = int(rng.integers(min_dist, 31)) if pad and rng.random() < 0.5 else min_dist
            lit_lens = (lit_lens + [0] * 286)[:n_lit]
            dist_lens = (dist_lens + [0] * 30)[:n_dist]
            cl_seq = rle_random(rng, lit_lens + dist_lens)
        if check:
            assert 257 <= n_lit <= 286 and 1 <= n_dist <= 30
            assert expand_cl_seq(cl_seq) == lit_lens + dist_lens and cl_seq[0][0] != 16
            assert lit_lens[256] and (kraft(lit_lens) == 32768 or [n for n in lit_lens if n] == [1])
            assert kraft(dist_lens) in (0, 32768) or [n for n in dist_lens if n] == [1]
        if [n for n in dist_lens if n] == [1]:
            self.stats["single_dist_code"] += 1
        if cl_lens is None:
            used_cl = {s for s, _ in cl_seq}
            if len(used_cl) == 1:
                used_cl.add((min(used_cl) + 1) % 19)  # the code-length code has to be complete
            cl_lens = random_code_lengths(rng, used_cl, 19, 7, skew, extra)
        if check:
            assert kraft(cl_lens) == 32768 and max(cl_lens) <= 7
        min_cl = max([4] + [k + 1 for k, s in enumerate(CL_ORDER) if cl_lens[s]])
        if n_cl is None:
            n_cl = int(rng.integers(min_cl, 20)) if pad and rng.random() < 0.5 else min_cl
        assert min_cl <= n_cl <= 19
        for key, v in (("n_lit", n_lit), ("n_dist", n_dist), ("n_cl", n_cl)):
            self.stats[key].add(v)
        # what the sequence holds
        at, prev = 0, None
        for sym, x in cl_seq:
            rep = 1 if sym < 16 else (3 if sym in (16, 17) else 11) + x
            if sym == 16:
                self.stats["rep16_cross"] += at < n_lit < at + rep
                self.stats["rep16_after16"] += prev == 16
                self.stats["rep16_after_zeros"] += prev in (17, 18)
            at, prev = at + rep, sym
        self._header(final, 2, "dynamic")
        m = self.marks[-1]
        m["hlit"], m["hdist"], m["hclen"] = self.w.pos, self.w.pos + 5, self.w.pos + 10
        self.w.bits(n_lit - 257, 5)
        self.w.bits(n_dist - 1, 5)
        self.w.bits(n_cl - 4, 4)
        m["cl_lens"] = self.w.pos
        for k in range(n_cl):
            self.w.bits(cl_lens[CL_ORDER[k]], 3)
        m["cl_seq"] = self.w.pos
        cl_codes = canonical_codes(cl_lens)
        for sym, x in cl_seq:
            assert cl_lens[sym]
            self.w.code(cl_codes[sym], cl_lens[sym])
            if sym >= 16:
                self.w.bits(x, {16: 2, 17: 3, 18: 7}[sym])
        m["body"] = self.w.pos
        self._body(tokens, lit_lens, dist_lens, emit_eob)
        return self

    def _body(self, tokens, lit_lens, dist_lens, emit_eob):
        w, st, text = self.w, self.stats, self.text
        lit_codes = [reverse_bits(c, n) for c, n in zip(canonical_codes(lit_lens), lit_lens)]  # as they go into the stream
        dist_codes = [reverse_bits(c, n) for c, n in zip(canonical_codes(dist_lens), dist_lens)]
        mc = st["maxcode"]
        for k, t in enumerate(tokens):
            if t[0] == "L":
                b = t[1]
                assert lit_lens[b]
                w.bits(lit_codes[b], lit_lens[b])
                mc["lit"] = max(mc["lit"], lit_lens[b])
                text.append(b)
            elif t[0] == "M":
                length, dist = t[1], t[2]
                alt = len(t) > 3 and t[3]
                assert 3 <= length <= 258 and 1 <= dist <= 32768
                sym, xb, xv = length_symbol(length, alt)
                assert lit_lens[sym]
                w.bits(lit_codes[sym], lit_lens[sym])
                w.bits(xv, xb)
                mc["len"] = max(mc["len"], lit_lens[sym])
                dsym, xb, xv = distance_symbol(dist)
                assert dist_lens[dsym]
                w.bits(dist_codes[dsym], dist_lens[dsym])
                w.bits(xv, xb)
                mc["dist"] = max(mc["dist"], dist_lens[dsym])
                st["alt258"] += bool(alt)
                st["first_match"] += k == 0
                st["overlap"] += dist < length
                for wd in WINDOWS:
                    if abs(dist - wd) <= 1:
                        st["wclass"][(wd, dist - wd)] += 1
                if dist > len(text):
                    self.broken = True  # an invalid stream on purpose: the text ends here
                elif not self.broken:
                    src = len(text) - dist
                    if dist >= length:
                        text += text[src : src + length]
                    else:
                        piece = bytes(text[src:])
                        text += (piece * (length // dist + 1))[:length]
            elif t[0] == "S":
                w.bits(lit_codes[t[1]], lit_lens[t[1]])
                self.broken = True
            elif t[0] == "D":
                w.bits(dist_codes[t[1]], dist_lens[t[1]])
                self.broken = True
            else:
                raise ValueError(t)
        if emit_eob:
            w.bits(lit_codes[256], lit_lens[256])
            mc["eob"] = max(mc["eob"], lit_lens[256])
        self.marks[-1]["end"] = w.pos

    def raw(self):
        return self.w.getvalue()

    def bit_length(self):
        return self.w.pos


# ---- LZ77 parses -------------------------------------------------------------------------------------

AWKWARD_LENGTHS = [3, 3, 4, 5, 8, 13, 31, 63, 64, 65, 66, 128, 129, 200, 257, 258, 258]


def tokenize(text, rng, start=0, end=None, p_literal=0.3, lengths=AWKWARD_LENGTHS):
    """A random LZ77 parse of text[start:end] (matches may reach back before `start`): at each position
    a literal, or a length from `lengths` and a source found with bytes.rfind / bytes.find inside the
    last 32 768 bytes -- the nearest or the farthest one; a source may overlap the match itself."""
    end = len(text) if end is None else end
    toks, i = [], start
    while i < end:
        if i == 0 or rng.random() < p_literal:
            toks.append(("L", text[i]))
            i += 1
            continue
        want = min(int(lengths[int(rng.integers(len(lengths)))]), end - i)
        lo = max(0, i - 32768)
        for n in (want, min(want, 12), 3):
            if n < 3 or n > end - i:
                continue
            needle = text[i : i + n]
            j = text.rfind(needle, lo, i + n - 1) if rng.random() < 0.6 else text.find(needle, lo, i + n - 1)
            if j >= 0:
                toks.append(("M", n, i - j, n == 258 and rng.random() < 0.5))
                i += n
                break
        else:
            toks.append(("L", text[i]))
            i += 1
    return toks


def random_tokens(rng, pos, room, alphabet):
    """`room` bytes of literals and matches behind `pos` bytes of history.  Lengths and distances come
    from lists that hold the awkward values, clipped to what exists."""
    toks, n = [], 0
    while n < room:
        h = pos + n
        length = min(int(AWKWARD_LENGTHS[int(rng.integers(len(AWKWARD_LENGTHS)))]), room - n)
        if h == 0 or length < 3 or rng.random() < 0.3:
            toks.append(("L", int(alphabet[int(rng.integers(len(alphabet)))])))
            n += 1
            continue
        cand = [1, 2, 3, 63, 64, 65, length - 1, length, length + 1, h, int(rng.integers(1, h + 1))]
        cand += [w + o for w in WINDOWS for o in (-1, 0, 1)] * 2
        cand = [d for d in cand if 1 <= d <= min(h, 32768)]
        toks.append(("M", length, cand[int(rng.integers(len(cand)))], length == 258 and rng.random() < 0.5))
        n += length
    return toks


def random_member(rng, size, skew, text=None):
    """A member of `size` bytes of text as a random mix of stored, fixed and dynamic blocks of random
    sizes; `text` given: an encoding of exactly that text through `tokenize`."""
    m = Member()
    size = len(text) if text is not None else size
    alphabet = rng.integers(0, 256, size=int(rng.choice([2, 5, 40, 256])))
    kinds = ["stored", "fixed", "dynamic", "dynamic"]
    pos = 0
    while True:
        left = size - pos
        n = min(left, int(rng.choice([left, left, int(rng.integers(0, left + 1)), int(rng.integers(0, 300)), 0])))
        final = pos + n == size and (n > 0 or rng.random() < 0.5 or size == 0)
        kind = kinds[int(rng.integers(len(kinds)))]
        if kind == "stored":
            n = min(n, 65535)
            final = final and pos + n == size
            m.stored(text[pos : pos + n] if text is not None else bytes(rng.integers(0, 256, size=n, dtype=np.uint8)), final)
        else:
            toks = tokenize(text, rng, pos, pos + n) if text is not None else random_tokens(rng, pos, n, alphabet)
            if kind == "fixed":
                m.fixed(toks, final)
            else:
                m.dynamic(toks, final, rng, skew=skew, deep_eob=0.15)
        pos += n
        assert len(m.text) == pos
        if final:
            break
    assert text is None or bytes(m.text) == text
    return m


# ---- the BGZF container ------------------------------------------------------------------------------


def bgzf_member(raw, text):
    """A raw stream as a BGZF member (SAM spec 4.1), as write_bgzf in test_ingest_native.py wraps zlib's."""
    bsize = 12 + 6 + len(raw) + 8
    assert bsize <= 65536 and len(text) <= 65536
    head = b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
    return head + raw + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text))


def write_bgzf_file(path, members):
    """`members`: (raw stream, text) pairs; the empty EOF member is added."""
    with open(path, "wb") as f:
        for raw, text in members:
            f.write(bgzf_member(raw, text))
        f.write(bgzf_member(Member().fixed([], True).raw(), b""))


# ---- the corpora the tests share (fixed seeds) ----------------------------------------------------------


def vcf_like(rng, n):
    """VCF-shaped text (the generator of test_inflate_device.py, kept here so that the CPU test needs no GPU module)."""
    calls = np.array([b"0|0", b"0|1", b"1|0", b"1|1", b".|."])
    out, pos = bytearray(), 0
    while len(out) < n:
        pos += int(rng.integers(1, 900))
        row = calls[rng.choice(5, size=400, p=[0.8, 0.07, 0.07, 0.055, 0.005])]
        out += b"21\t%d\trs%d\tA\tG\t.\tPASS\tAC=%d;AN=800\tGT\t" % (pos, pos, int(rng.integers(0, 800))) + b"\t".join(row) + b"\n"
    return bytes(out[:n])


def _rand(rng, n):
    return bytes(rng.integers(0, 256, size=n, dtype=np.uint8))


def _chain(n_syms, order, depth=15):
    """Chain code lengths 1, 2, ..., depth-1, depth, depth for the symbols in `order` (Kraft sum 1)."""
    lens = [0] * n_syms
    d = list(range(1, depth)) + [depth, depth]
    assert len(order) == len(d)
    for s, n in zip(order, d):
        lens[s] = n
    return lens


_CACHE = {}


def _cached(fn):
    def get():
        if fn.__name__ not in _CACHE:
            _CACHE[fn.__name__] = fn()
        return _CACHE[fn.__name__]

    get.__name__ = fn.__name__
    get.__doc__ = fn.__doc__
    return get


@_cached
def directed_cases():
    """[(name, raw stream, text, stats)]: one member per case, each from explicit tokens."""
    rng = np.random.default_rng(20240)
    cases = []

    def add(name, m):
        cases.append((name, m.raw(), bytes(m.text), m.stats))

    def tail(length):
        return [("M", length, length), ("M", 258, 1), ("L", 0x5A)]

    # the LDS / HBM boundary of every instantiation: d = W - 1, W, W + 1 (the source slot aliases the destination modulo W)
    for w in WINDOWS:
        for off in (-1, 0, 1):
            d = w + off
            if d > 32768:
                continue
            for length in (3, 64, 65, 258):
                m = Member().stored(_rand(rng, d + int(rng.integers(0, 3)) * int(rng.integers(0, 700))))
                pad = len(m.text) - d  # the match starts `pad` bytes into the stored text
                blk = [("M", length, d)] + tail(length)
                m.fixed(blk, True) if (length + off) % 2 else m.dynamic(blk, True, rng)
                add("boundary W=%d d=W%+d len=%d pad=%d" % (w, off, length, pad), m)
    # matches that read their own output
    for d in (1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 257):
        for length in (3, 63, 64, 65, 128, 129, 257, 258):
            m = Member().stored(_rand(rng, d + int(rng.integers(0, 40))))
            m.fixed([("M", length, d, length == 258 and d % 2 == 1), ("L", 1), ("M", length, d)], True)
            add("overlap d=%d len=%d" % (d, length), m)
    # the same far match with 0, 1, 255 bytes not yet flushed in front of it
    for d in (5000, 9000, 17000):
        for r in (0, 1, 255):
            m = Member().stored(_rand(rng, 17408 + r)).fixed([("M", 100, d), ("M", 258, d), ("L", 7)], True)
            add("far d=%d unflushed=%d" % (d, r), m)
    # ... and with its output crossing the wrap of the window
    for w in WINDOWS:
        for back in (1, 3, 200):
            d = w + 37 if w < 32768 else w - back
            n = 2 * w - back if w < 32768 else w - back
            m = Member().stored(_rand(rng, n)).fixed([("M", 258, d), ("M", 258, d), ("L", 9), ("M", 5, d)], True)
            add("wrap W=%d out_pos=%d d=%d" % (w, n, d), m)
    # a far match as the first symbol of a fixed / dynamic block directly after a stored block
    for d in (4097, 8193, 16385, 20000):
        for dyn in (False, True):
            m = Member().stored(_rand(rng, 21000))
            toks = [("M", 258, d), ("L", 3), ("M", 4, 1)]
            m.dynamic(toks, True, rng, skew=0.9) if dyn else m.fixed(toks, True)
            add("far first symbol d=%d %s" % (d, "dynamic" if dyn else "fixed"), m)
    # two far matches in a row: the second one's source follows, is, or precedes the first one's source --
    # the text just behind the edge of the window, the youngest a far match can read
    for w in (4096, 8192, 16384):
        for d2 in (w + 1, w + 1 + 258, w + 1 + 516):
            m = Member().stored(_rand(rng, w + 900)).fixed([("L", 1)] * 77 + [("M", 258, w + 1), ("M", 258, d2), ("L", 2)], True)
            add("two far matches W=%d d2=%d" % (w, d2), m)
    # the last match ends exactly at 65 536; the last literal sits at offset 65 535
    m = Member().stored(_rand(rng, 65535)).fixed([("L", 0xEE)], True)
    add("last literal at 65535", m)
    for d in (1, 4096, 4097, 32768):
        m = Member().stored(_rand(rng, 40000)).stored(_rand(rng, 65536 - 258 - 40000)).fixed([("M", 258, d)], True)
        add("last match ends at 65536 d=%d" % d, m)
    # ---- header edges ----
    # distance codes longer than the 8-bit primary table: a chain over all 30 symbols, the deep ones used
    order = [int(s) for s in rng.permutation(30)][:16]
    dl = _chain(30, order)
    toks = [("L", 65)] * 3
    m = Member().stored(_rand(rng, 33000))
    for s in order[8:]:
        toks += [("M", 9, min(DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1, 33000)), ("L", 66)]
    add("distance codes of 9-15 bits", m.dynamic(toks, True, rng, dist_lens=dl))
    # length symbols and the end-of-block symbol with 11-15-bit codes
    lit_order = [65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 257, 265, 270, 284, 256, 285]
    ll = _chain(286, lit_order)
    toks = [("L", 65 + k) for k in range(10)] + [("M", 3, 1), ("M", 12, 2), ("M", 25, 3), ("M", 257, 4), ("M", 258, 5), ("M", 258, 10, True)]
    add("length and end-of-block codes of 11-15 bits", Member().dynamic(toks, True, rng, lit_lens=ll, dist_lens=[3] * 8 + [0] * 22))
    # the most bits between two refills: a 15-bit length code + 5 extra bits, a 15-bit distance code + 13 extra bits
    ll = _chain(286, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 284, 256])
    dl = _chain(30, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 29, 28])
    m = Member().stored(_rand(rng, 32768))
    toks = [("M", 257, 32768), ("M", 258, 32768, True), ("L", 0), ("M", 227, 24577), ("M", 257, 16385 + 8191), ("M", 250, 32767)]
    add("15+5 and 15+13 bits in one match", m.dynamic(toks, True, rng, lit_lens=ll, dist_lens=dl))
    # length 258 as symbol 284 with extra bits 31 (fixed and dynamic)
    add("258 as 284+31 fixed", Member().fixed([("L", 1), ("L", 2), ("M", 258, 2, True), ("M", 258, 1, True), ("M", 258, 258, True)], True))
    add("258 as 284+31 dynamic", Member().dynamic([("L", 1), ("M", 258, 1, True), ("M", 258, 259, True)], True, rng, skew=0.5))
    # a single distance code of length 1 (incomplete but legal), on symbol 0 and on a symbol with extra bits
    for ds, d in ((0, 1), (9, 30)):
        dl = [0] * 30
        dl[ds] = 1
        toks = [("L", k) for k in range(40)] + [("M", 30, d), ("M", 3, d)]
        add("single distance code on symbol %d" % ds, Member().dynamic(toks, True, rng, dist_lens=dl, pad=False))
    # HLIT / HDIST / HCLEN at their minima: 257 literal/length lengths, one distance length (zero), and the five
    # code-length lengths a block needs at the least (16 17 18 0 8: with four, every length would be zero)
    seq = [(0, 0)] + [(8, 0)] * 256 + [(0, 0)]
    cl = [0] * 19
    cl[0] = cl[8] = 1
    m = Member().dynamic([("L", 1 + k) for k in range(255)], True, cl_seq=seq, n_lit=257, n_dist=1, n_cl=5, cl_lens=cl)
    add("HLIT HDIST HCLEN minima", m)
    # ... and at their maxima: 286, 30, 19 (symbol 285, distance symbol 29 and code-length symbol 15 in use)
    ll = _chain(286, [256, 285, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45])
    dl = _chain(30, [29, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14])
    m = Member().stored(_rand(rng, 30000))
    m.dynamic([("L", 45), ("M", 258, 29999), ("L", 32)], True, rng, lit_lens=ll, dist_lens=dl, n_lit=286, n_dist=30, n_cl=19, pad=False)
    add("HLIT HDIST HCLEN maxima", m)
    m = Member().dynamic([("L", 45), ("L", 32)], True, rng, lit_lens=ll, n_lit=286, n_dist=30, n_cl=19, pad=False)
    add("HLIT HDIST HCLEN maxima by padding", m)
    # repeat code 16 from the literal lengths into the distance lengths; 16 after 16; 16 after 17 and after 18:
    #   lengths 0-5 zero (17 then 16), 6-19 zero (18 then 16), 20-147 eight (8, then 16 after 16 ...), 148-255 zero,
    #   256 and 257 two, distance 0-3 two (one 16 covers 257 and all four distance lengths)
    seq = [(17, 0), (16, 0), (18, 0), (16, 0), (8, 0)] + [(16, 3)] * 21 + [(8, 0)] + [(18, 108 - 11)] + [(2, 0), (16, 2)]
    assert expand_cl_seq(seq) == [0] * 20 + [8] * 128 + [0] * 108 + [2] * 6
    toks = [("L", 20), ("L", 147), ("L", 99), ("M", 3, 1), ("M", 3, 4), ("M", 3, 3), ("M", 3, 2)]
    m = Member().dynamic(toks, True, rng, cl_seq=seq, n_lit=258, n_dist=4)
    assert m.stats["rep16_cross"] == 1 and m.stats["rep16_after16"] >= 20 and m.stats["rep16_after_zeros"] == 2
    add("16 across the boundary, after 16, after 17 and 18", m)
    # a stored block at each of the eight bit offsets behind a Huffman block: k nine-bit literals in front
    for k in range(8):
        for empty in (True, False):
            m = Member().fixed([("L", 200 + k)] * k)
            assert m.bit_length() % 8 == (10 + 9 * k) % 8
            m.stored(b"" if empty else _rand(rng, 300 + k))
            m.fixed([("M", 3, 1)] if k else [("L", 5)], True) if k % 2 == 0 else m.stored(_rand(rng, k), True)
            add("%s stored block at bit offset %d" % ("empty" if empty else "a", (10 + 9 * k) % 8), m)
    # a match that is the first symbol of a block and reaches back into a stored block, through an empty fixed block
    m = Member().stored(_rand(rng, 500)).fixed([]).fixed([("M", 258, 500), ("M", 100, 758)], True)
    add("first symbol reaches into a stored block", m)
    # a final block that ends on the last bit of the stream, and one that ends inside its last byte
    m = Member().fixed([("L", 200)] * 6, True)
    assert m.bit_length() % 8 == 0
    add("final block ends on a byte boundary", m)
    m = Member().fixed([("L", 1)], True)
    assert m.bit_length() % 8 == 2
    add("final block ends mid-byte", m)
    m = Member().stored(b"abc").dynamic([("M", 3, 3)], True, rng)
    add("final dynamic block", m)
    return cases


CORPUS_SIZES = (0, 1, 255, 256, 257, 4096, 4097, 65535, 65536)
CORPUS_MEMBERS = 300
WINDOW_SLICE = [3 * k + k % 3 for k in range(100)]  # the 100 members that also run on the other three instantiations


@_cached
def seeded_corpus():
    """[(raw stream, text, stats)]: CORPUS_MEMBERS members from random_member, every third one an
    encoding of VCF-like text through tokenize, every fourth size drawn freely."""
    rng = np.random.default_rng(777)
    base = vcf_like(rng, 1 << 19)
    out = []
    for i in range(CORPUS_MEMBERS):
        size = int(rng.integers(0, 65537)) if i % 4 == 3 else int(CORPUS_SIZES[int(rng.integers(len(CORPUS_SIZES)))])
        skew = float([0.0, 0.5, 0.95][i % 3 if i % 5 else 2])
        if i % 3 == 1 or i % 7 == 0:
            o = int(rng.integers(0, len(base) - size + 1))
            m = random_member(rng, size, skew, text=base[o : o + size])
        else:
            m = random_member(rng, size, skew)
        raw = m.raw()
        assert len(raw) <= 1 << 17 and len(m.text) == size
        m.stats["from_text"] = i % 3 == 1 or i % 7 == 0
        out.append((raw, bytes(m.text), m.stats))
    return out


@_cached
def invalid_cases():
    """[(name, raw stream, declared text, bad)]: a valid member with exactly one field damaged, one or
    more per class the kernel has a branch for.  The declared text gives ISIZE and the CRC of the
    trailer.  `bad` is False for the few controls: the valid member the damaged ones next to it derive from."""
    rng = np.random.default_rng(4242)
    cases = []
    head = _rand(rng, 300)
    toks = [("L", int(b)) for b in _rand(rng, 60)] + [("M", 30, 200), ("M", 258, 1), ("L", 3), ("M", 10, 360)]

    def valid(kind="fixed", **kw):
        m = Member().stored(head)
        m.fixed(toks, True) if kind == "fixed" else m.dynamic(toks, True, np.random.default_rng(1), **kw)
        return m

    text = bytes(valid().text)
    # block type 3, as the last block and as the first
    for kind in ("fixed", "dynamic"):
        m = valid(kind)
        cases.append(("block type 3 (%s)" % kind, patch_bits(m.raw(), m.marks[1]["btype"], 2, 3), text, True))
    m = valid()
    cases.append(("block type 3 (first)", patch_bits(m.raw(), m.marks[0]["btype"], 2, 3), text, True))
    # LEN != ~NLEN: one bit of NLEN, one bit of LEN
    cases.append(("NLEN bit flipped", patch_bits(m.raw(), m.marks[0]["nlen"], 16, (300 ^ 0xFFFF) ^ 0x0100), text, True))
    cases.append(("LEN bit flipped", patch_bits(m.raw(), m.marks[0]["len"], 16, 300 ^ 0x0001), text, True))
    # HLIT > 286, HDIST > 30
    m = valid("dynamic", pad=False)
    for v in (30, 31):
        cases.append(("HLIT field %d" % v, patch_bits(m.raw(), m.marks[1]["hlit"], 5, v), text, True))
        cases.append(("HDIST field %d" % v, patch_bits(m.raw(), m.marks[1]["hdist"], 5, v), text, True))
    # repeat code 16 as the first code length; a repeat that overruns HLIT + HDIST
    lits = [("L", 20 + k) for k in range(100)]
    seq_ok = [(17, 0), (0, 0), (0, 0), (0, 0)] + [(18, 3)] + [(8, 0)] * 128 + [(18, 97)] + [(2, 0)] * 2 + [(1, 0)]
    assert expand_cl_seq(seq_ok) == [0] * 20 + [8] * 128 + [0] * 108 + [2, 2, 1]
    cl = [0] * 19
    cl[0], cl[1], cl[2], cl[8], cl[16], cl[17], cl[18] = 3, 3, 4, 1, 4, 4, 4
    good = Member().stored(head).dynamic(lits, True, cl_seq=seq_ok, n_lit=258, n_dist=1, cl_lens=cl)
    cases.append(("(control: the valid form of the next three)", good.raw(), bytes(good.text), False))
    m = Member().stored(head).dynamic(lits, True, cl_seq=[(16, 0)] + seq_ok[1:], n_lit=258, n_dist=1, cl_lens=cl, check=False)
    cases.append(("16 as the first code length", m.raw(), bytes(good.text), True))
    m = Member().stored(head).dynamic(lits, True, cl_seq=seq_ok[:-3] + [(2, 0), (16, 0)], n_lit=258, n_dist=1, cl_lens=cl, check=False)
    cases.append(("16 overruns the total", m.raw(), bytes(good.text), True))
    m = Member().stored(head).dynamic(lits, True, cl_seq=seq_ok[:-4] + [(18, 127)], n_lit=258, n_dist=1, cl_lens=cl, check=False)
    cases.append(("18 overruns the total", m.raw(), bytes(good.text), True))
    # no end-of-block code: the length of symbol 256 zeroed (the literals are complete on their own here)
    cl2 = [0] * 19
    cl2[0] = cl2[8] = 1
    m = Member().stored(head).dynamic([("L", 1 + k) for k in range(200)], True, cl_seq=[(8, 0)] * 256 + [(0, 0)] * 3,
                                      n_lit=258, n_dist=1, cl_lens=cl2, check=False, emit_eob=False)  # fmt: skip
    cases.append(("no end-of-block code", m.raw(), head + bytes(range(1, 201)), True))
    # over-subscribed lengths: one length of a complete code shortened by one -- literal/length, distance, code-length code
    ll = [0] * 286
    for s in range(20, 148):
        ll[s] = 8
    ll[256], ll[257], ll[258] = 2, 3, 3
    dl = [2, 2, 2, 2] + [0] * 26
    body = lits + [("M", 3, 1), ("M", 4, 4)]
    ok = Member().stored(head).dynamic(body, True, np.random.default_rng(2), lit_lens=ll, dist_lens=dl)
    cases.append(("(control: the valid form of the next three)", ok.raw(), bytes(ok.text), False))
    bad_ll = list(ll)
    bad_ll[258] = 2
    m = Member().stored(head).dynamic(body, True, np.random.default_rng(2), lit_lens=bad_ll, dist_lens=dl, check=False)
    cases.append(("over-subscribed literal/length lengths", m.raw(), bytes(ok.text), True))
    bad_ll = list(ll)
    bad_ll[77] = 7
    m = Member().stored(head).dynamic(body, True, np.random.default_rng(2), lit_lens=bad_ll, dist_lens=dl, check=False)
    cases.append(("over-subscribed literal/length lengths (long code)", m.raw(), bytes(ok.text), True))
    m = Member().stored(head).dynamic(body, True, np.random.default_rng(2), lit_lens=ll, dist_lens=[2, 2, 2, 1] + [0] * 26, check=False)
    cases.append(("over-subscribed distance lengths", m.raw(), bytes(ok.text), True))
    bad_cl = list(cl)
    bad_cl[17] = 3
    m = Member().stored(head).dynamic(lits, True, cl_seq=seq_ok, n_lit=258, n_dist=1, cl_lens=bad_cl, check=False)
    cases.append(("over-subscribed code-length code", m.raw(), bytes(good.text), True))
    # length symbols 286 / 287 and distance symbols 30 / 31 in a fixed block
    for s in (286, 287):
        m = Member().stored(head).fixed(toks + [("S", s), ("D", 0), ("L", 1)], True)
        cases.append(("fixed block: length symbol %d" % s, m.raw(), text + b"\x01" * 4, True))
    for s in (30, 31):
        m = Member().stored(head).fixed(toks + [("S", 257), ("D", s), ("L", 1)], True)
        cases.append(("fixed block: distance symbol %d" % s, m.raw(), text + b"\x01" * 4, True))
    # a distance beyond the text so far: by one, as the first symbol of the member, and far
    m = Member().stored(head).fixed([("L", 1), ("M", 3, 302), ("L", 2)], True)
    cases.append(("distance one beyond the text", m.raw(), head + b"\x01\x01\x01\x01\x02", True))
    m = Member().fixed([("M", 3, 1), ("L", 2)], True)
    cases.append(("match as the first symbol of the member", m.raw(), b"\x02\x02\x02\x02", True))
    m = Member().stored(head).dynamic([("L", 1), ("M", 258, 32768), ("L", 2)], True, np.random.default_rng(3))
    cases.append(("distance 32768 over 301 bytes", m.raw(), head + b"\x01" * 259 + b"\x02", True))
    # text beyond ISIZE (valid DEFLATE): the overrun by a literal, by a match, by a stored block
    m = Member().stored(head).fixed(toks + [("L", 9)], True)
    cases.append(("text beyond ISIZE: literal", m.raw(), bytes(m.text[:-1]), True))
    m = Member().stored(head).fixed(toks + [("M", 258, 100)], True)
    cases.append(("text beyond ISIZE: match", m.raw(), bytes(m.text[:-1]), True))
    cases.append(("text beyond ISIZE: match, by 257", m.raw(), bytes(m.text[:-257]), True))
    m = Member().fixed(toks[:60]).stored(head, True)
    cases.append(("text beyond ISIZE: stored", m.raw(), bytes(m.text[:-1]), True))
    cases.append(("text beyond ISIZE: ISIZE 0", m.raw(), b"", True))
    # ISIZE larger than the text
    m = valid()
    cases.append(("ISIZE larger than the text by 1", m.raw(), text + b"\x03", True))
    cases.append(("ISIZE larger than the text by 300", m.raw(), text + head, True))
    m = valid("dynamic")
    cases.append(("ISIZE larger than the text (dynamic)", m.raw(), text + b"\x03", True))
    return cases


CRC_SIZES = (0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513)


@_cached
def crc_cases():
    """{size: [(raw stream, text)] * 8}: eight different members of every size in CRC_SIZES."""
    rng = np.random.default_rng(99)
    out = {}
    for n in CRC_SIZES:
        out[n] = []
        for k in range(8):
            m = random_member(rng, n, 0.5)
            out[n].append((m.raw(), bytes(m.text)))
    return out


def product_members(text, rng):
    """`text` cut at ragged sizes, every piece encoded through tokenize with a random block mix -- a few
    pieces pure stored, a few pure fixed -- as (raw stream, text) pairs that fit a BGZF member."""
    out, pos, k = [], 0, 0
    while pos < len(text):
        n = min(len(text) - pos, int(rng.choice([1, 17, 300, 4097, 9000, int(rng.integers(1, 30000))])))
        piece = text[pos : pos + n]
        if k % 7 == 3:
            m = Member().stored(piece, True)
        elif k % 7 == 5:
            m = Member().fixed(tokenize(piece, rng), True)
        else:
            m = random_member(rng, n, float(rng.choice([0.0, 0.5, 0.95])), text=piece)
        assert bytes(m.text) == piece
        out.append((m.raw(), piece))
        pos += n
        k += 1
    return out
