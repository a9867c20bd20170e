"""tests/deflate_builder.py proven right before it judges a kernel: zlib's decoder agrees with the
builder's own text on every member of every corpus the GPU tests use (same functions, same seeds),
rejects every member that is damaged on purpose, and the corpora hold what they claim to hold."""

import zlib

import numpy as np

import deflate_builder as db


def zlib_inflate(raw):
    """(text, eof, unused) of a raw DEFLATE stream; raises zlib.error for an invalid one."""
    d = zlib.decompressobj(-15)
    text = d.decompress(raw)
    return text, d.eof, d.unused_data


def assert_valid(raw, text, what):
    got, eof, unused = zlib_inflate(raw)
    assert got == text, (what, len(got), len(text))
    assert eof and unused == b"", (what, eof, len(unused))


def test_bit_writer_and_code_tables():
    w = db.BitWriter()
    w.bits(1, 1)
    w.bits(2, 2)
    w.code(0b110, 3)  # MSB first: goes in as 011
    w.bits(0x1FF, 9)
    assert w.pos == 15 and w.getvalue() == bytes([0b11011101, 0b01111111])
    assert db.patch_bits(w.getvalue(), 1, 2, 3) == bytes([0b11011111, 0b01111111])
    for length in range(3, 259):
        s, xb, xv = db.length_symbol(length)
        assert db.LEN_BASE[s - 257] + xv == length and xv < (1 << xb) or (length == 258 and s == 285)
    assert db.length_symbol(258, True) == (284, 5, 31) and db.length_symbol(258) == (285, 0, 0)
    for d in list(range(1, 600)) + [4096, 4097, 24576, 24577, 32767, 32768]:
        s, xb, xv = db.distance_symbol(d)
        assert db.DIST_BASE[s] + xv == d and xv < (1 << max(xb, 1))
    # RFC 1951 3.2.2's example
    assert db.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [0b010, 0b011, 0b100, 0b101, 0b110, 0b00, 0b1110, 0b1111]
    rng = np.random.default_rng(1)
    for n, depth, skew in ((2, 15, 0.0), (19, 7, 0.9), (286, 15, 0.0), (286, 15, 0.95), (30, 15, 1.0), (128, 7, 0.5)):
        d = db.random_prefix_depths(rng, n, depth, skew)
        assert len(d) == n and max(d) <= depth and db.kraft(d) == 32768
    assert max(db.random_prefix_depths(rng, 40, 15, 1.0)) == 15
    lens = [0, 0, 0, 0, 0, 5, 5, 5, 5, 5, 5, 5, 5, 5, 3] + [0] * 150 + [7] * 9
    for _ in range(50):
        assert db.expand_cl_seq(db.rle_random(rng, lens)) == lens


def test_directed_members_are_what_zlib_reads():
    cases = db.directed_cases()
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    for name, raw, text, _ in cases:
        assert_valid(raw, text, name)
        assert len(text) <= 65536
    by = {c[0]: c for c in cases}
    # the matrix is whole: every instantiation's boundary, every length
    for w in db.WINDOWS:
        for off in (-1, 0, 1):
            if w + off <= 32768:
                for length in (3, 64, 65, 258):
                    hit = [c for c in cases if c[0].startswith("boundary W=%d d=W%+d len=%d " % (w, off, length))]
                    assert len(hit) == 1 and hit[0][3]["wclass"][(w, off)] == 1 and hit[0][3]["first_match"] == 1
    assert sum(n.startswith("overlap ") for n in names) == 88
    for d in (1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 257):
        for length in (3, 63, 64, 65, 128, 129, 257, 258):
            assert by["overlap d=%d len=%d" % (d, length)][3]["overlap"] == (2 if d < length else 0)
    # the header edges hold what their names say
    assert by["distance codes of 9-15 bits"][3]["maxcode"]["dist"] == 15
    st = by["length and end-of-block codes of 11-15 bits"][3]
    assert st["maxcode"]["len"] == 15 and st["maxcode"]["eob"] == 15 and st["alt258"] == 1
    st = by["15+5 and 15+13 bits in one match"][3]
    assert st["maxcode"]["len"] == 15 and st["maxcode"]["dist"] == 15 and st["maxcode"]["eob"] == 15 and st["alt258"] == 1
    assert by["258 as 284+31 fixed"][3]["alt258"] == 3 and by["258 as 284+31 dynamic"][3]["alt258"] == 2
    assert by["single distance code on symbol 0"][3]["single_dist_code"] == 1
    assert by["single distance code on symbol 9"][3]["single_dist_code"] == 1
    st = by["HLIT HDIST HCLEN minima"][3]
    assert (st["n_lit"], st["n_dist"], st["n_cl"]) == ({257}, {1}, {5})
    for n in ("HLIT HDIST HCLEN maxima", "HLIT HDIST HCLEN maxima by padding"):
        st = by[n][3]
        assert (st["n_lit"], st["n_dist"], st["n_cl"]) == ({286}, {30}, {19})
    st = by["16 across the boundary, after 16, after 17 and 18"][3]
    assert st["rep16_cross"] == 1 and st["rep16_after16"] >= 1 and st["rep16_after_zeros"] == 2
    for empty in ("empty", "a"):
        seen = set()
        for off in range(8):
            st = by["%s stored block at bit offset %d" % (empty, off)][3]
            seen |= {o for o in range(8) if st["stored_bit_offset"][o]}
        assert seen >= set(range(8)), seen
    assert by["first symbol reaches into a stored block"][3]["first_match"] == 1
    assert len(by["last literal at 65535"][2]) == 65536
    assert all(len(c[2]) == 65536 for c in cases if c[0].startswith("last match ends at 65536"))
    assert len(cases) >= 200


def test_seeded_corpus_is_what_zlib_reads_and_holds_what_it_claims():
    corpus = db.seeded_corpus()
    assert len(corpus) == db.CORPUS_MEMBERS >= 300
    for i, (raw, text, _) in enumerate(corpus):
        assert_valid(raw, text, i)
    stats = [c[2] for c in corpus]
    sizes = {len(c[1]) for c in corpus}
    assert sizes >= set(db.CORPUS_SIZES), sorted(sizes)[:20]
    assert sum(s["from_text"] for s in stats) * 3 >= len(corpus)
    report = {}
    for kind in ("stored", "fixed", "dynamic"):
        report["members with a %s block" % kind] = (sum(s["blocks"][kind] > 0 for s in stats), 50)
    report["members with >= 3 blocks"] = (sum(sum(s["blocks"].values()) >= 3 for s in stats), 50)
    report["members emitting a literal code > 10 bits"] = (sum(s["maxcode"]["lit"] > 10 for s in stats), 20)
    report["members emitting a length code > 10 bits"] = (sum(s["maxcode"]["len"] > 10 for s in stats), 20)
    report["members emitting a distance code > 8 bits"] = (sum(s["maxcode"]["dist"] > 8 for s in stats), 20)
    for a in ("lit", "len", "dist", "eob"):
        report["members emitting a 15-bit %s code" % a] = (sum(s["maxcode"][a] == 15 for s in stats), 1)
    for w in db.WINDOWS:
        for off in (-1, 0, 1):
            if w + off <= 32768:
                report["matches at distance %d%+d" % (w, off)] = (sum(s["wclass"][(w, off)] for s in stats), 5)
    for off in range(8):
        report["stored blocks at bit offset %d" % off] = (sum(s["stored_bit_offset"][off] for s in stats), 1)
    # the counters below have no bound set from outside: each asks that a feature the generator draws on purpose
    # (a tenth or more of its distance / length draws, or one run-length choice in a few) is there more than once
    report["overlapping matches"] = (sum(s["overlap"] for s in stats), 100)
    report["matches as the first symbol of a block"] = (sum(s["first_match"] for s in stats), 20)
    report["258 written as 284 + 31"] = (sum(s["alt258"] for s in stats), 20)
    report["16 across the literal/distance boundary"] = (sum(s["rep16_cross"] for s in stats), 1)
    report["16 after 16"] = (sum(s["rep16_after16"] for s in stats), 1)
    report["16 after 17 or 18"] = (sum(s["rep16_after_zeros"] for s in stats), 1)
    report["a single distance code"] = (sum(s["single_dist_code"] for s in stats), 1)
    short = {k: v for k, v in report.items() if v[0] < v[1]}
    assert not short, "counted, wanted at least: %r\nall counters: %r" % (short, report)
    # the slice that also runs on the other three instantiations is a fair one
    part = [stats[i] for i in db.WINDOW_SLICE]
    assert len(part) == 100 and len(set(db.WINDOW_SLICE)) == 100
    assert sum(s["from_text"] for s in part) >= 30
    for w in db.WINDOWS:
        for off in (-1, 0, 1):
            if w + off <= 32768:
                assert sum(s["wclass"][(w, off)] for s in part) >= 1, (w, off)


def test_invalid_members_are_invalid():
    cases = db.invalid_cases()
    kinds = " | ".join(c[0] for c in cases)
    for word in ("block type 3", "NLEN", "HLIT", "HDIST", "16 as the first", "overruns the total", "no end-of-block", "over-subscribed",
                 "length symbol 286", "length symbol 287", "distance symbol 30", "distance symbol 31", "beyond the text",
                 "text beyond ISIZE", "ISIZE larger"):  # fmt: skip
        assert word in kinds, word
    for name, raw, text, bad in cases:
        if not bad:
            assert_valid(raw, text, name)
            continue
        try:
            got, eof, _ = zlib_inflate(raw)
        except zlib.error:
            assert "ISIZE" not in name, name
            continue
        if "ISIZE" in name:  # valid DEFLATE: only the declared size is wrong
            assert eof and len(got) != len(text), name
            assert len(got) > len(text) if "beyond" in name else len(got) < len(text), name
        else:
            assert not eof or len(got) != len(text), name


def test_crc_and_product_members_are_what_zlib_reads():
    for n, members in db.crc_cases().items():
        assert len(members) == 8
        for raw, text in members:
            assert len(text) == n
            assert_valid(raw, text, n)
    rng = np.random.default_rng(5)
    text = db.vcf_like(rng, 150000)
    members = db.product_members(text, rng)
    assert b"".join(t for _, t in members) == text
    for raw, piece in members:
        assert_valid(raw, piece, len(piece))
        assert zlib.decompress(db.bgzf_member(raw, piece), 31) == piece
    assert db.bgzf_member(db.Member().fixed([], True).raw(), b"")[-8:] == b"\0" * 8
