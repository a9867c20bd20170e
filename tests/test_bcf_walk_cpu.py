"""The BCF route that finds the records on the GPU, on the host: the plain C++ twins of the two kernels
(``sai_bcf_chain_segments_host``, ``sai_bcf_record_heads_host``), ``sai_bcf_stitch`` and the feed, against the record
offsets tests/bcf_builder.py knows and against the host walk (``sai_bcf_stream_*``).  tests/test_bcf_walk_device.py
runs the kernels against the twins on the same streams."""

import ctypes as C
import re
import struct
import zlib

import numpy as np
import pytest

import abi_checks
import bcf_builder as B
import native_build
from conftest import ROOT
from test_bcf_cpu import FILES, REFUSED, _gt, anc_file, region_of, samples_of, small_bcf, vcf_text

MAX_HEADS = 8
DENSE = 1 << 30


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Stream:
    """The inflated stream of ``text`` as the builder writes it, and what the builder knows of every record: its
    offset, its fixed fields, REF and the first ALT, and where its GT array lies."""

    def __init__(self, text, on_record=None, **options):
        recs = []

        def hook(i, rec):
            if on_record is not None:
                on_record(i, rec)
            recs.append({k: (list(v) if isinstance(v, list) else v) for k, v in rec.items()})

        self.bytes = B.inflated_stream(text, on_record=hook, **options)
        lines = [ln for ln in text.split("\n") if ln]
        header = [ln for ln in lines if ln.startswith("#")]
        chroms = list(dict.fromkeys(ln.split("\t", 1)[0] for ln in lines if not ln.startswith("#")))
        _, self.contigs, self.strings, self.samples = B.build_header(header, chroms, options.get("idx", False), options.get("extra_before", False),
                                                                     options.get("extra_after", False))  # fmt: skip
        self.n_sample, self.gt_key = len(self.samples), self.strings["GT"]
        self.contig_defined = np.zeros(max(self.contigs.values()) + 1, dtype=np.uint8)
        self.contig_defined[list(self.contigs.values())] = 1
        sizes = [len(B.encode_record(r)) for r in recs]
        self.data_off = len(self.bytes) - sum(sizes)
        self.records, at = [], self.data_off
        for rec, size in zip(recs, sizes):
            shared = 24 + len(B.typed_string(rec["id"])) + sum(len(B.typed_string(a)) for a in rec["alleles"]) + len(B.typed_ints(rec["filter"]))
            gt, p = None, at + 8 + shared
            for f in rec["fmt"]:
                p += len(B.typed_int(f["key"])) + len(B.descriptor(f["type"], f["L"]))
                width = {B.INT8: 1, B.INT16: 2, B.INT32: 4, B.FLOAT: 4, B.CHAR: 1}[f["type"]]
                if f["key"] == self.gt_key and gt is None:
                    gt = (p, width, f["L"])
                p += len(f["payload"]) if "payload" in f else width * len(f["values"])
            alleles = rec["alleles"]
            self.records.append(dict(off=at, l_shared=shared, l_indiv=size - 8 - shared, chrom=rec["chrom"], pos0=rec["pos0"], n_allele=rec["n_allele"],
                                     n_fmt=len(rec["fmt"]), ref=alleles[0].encode(), alt=alleles[1].encode() if len(alleles) > 1 else b".", gt=gt))  # fmt: skip
            at += size


def host_kernels(data, n_bytes, seg_bytes, max_heads, st):
    """(chains, seg_info) of the host twin of kernel A."""
    from sai_amd import _ffi_bcf_device as D

    lib = D.load_host()
    n_seg = -(-n_bytes // seg_bytes)
    chains, info = np.full(n_seg * max_heads, 0x5A, dtype=np.uint8).repeat(16).view(D.CHAIN), np.full(n_seg, -7, dtype=np.int32)
    assert lib.sai_bcf_chain_segments_host(ptr(data), n_bytes, seg_bytes, max_heads, ptr(st.contig_defined), len(st.contig_defined), st.n_sample,
                                           ptr(chains), ptr(info)) == 0, lib.sai_last_error()  # fmt: skip
    return chains, info


def host_heads(data, n_bytes, seg_bytes, seg_entry, seg_first, carry_from, n_records, gt_key, want_gt):
    from sai_amd import _ffi_bcf_device as D

    lib = D.load_host()
    heads = np.zeros(n_records, dtype=D.HEAD)
    assert lib.sai_bcf_record_heads_host(ptr(data), n_bytes, seg_bytes, ptr(seg_entry), ptr(seg_first), carry_from, n_records, gt_key, int(want_gt),
                                         ptr(heads)) == 0, lib.sai_last_error()  # fmt: skip
    return heads


def walk(st, seg_bytes, data=None, e0=None, max_heads=MAX_HEADS, want_gt=True, kernels=host_kernels, heads_of=host_heads):
    """Kernel A, the stitch and kernel B over one batch: a dict of everything they return."""
    from sai_amd import _ffi_bcf_device as D

    lib = D.load_host()
    data = np.frombuffer(st.bytes if data is None else data, dtype=np.uint8).copy()
    n_bytes, e0 = len(data), st.data_off if e0 is None else e0
    chains, info = kernels(data, n_bytes, seg_bytes, max_heads, st)
    n_seg = len(info)
    seg_entry, seg_first = np.empty(n_seg, dtype=np.int64), np.empty(n_seg, dtype=np.int64)
    n_records, carry_from, verdict = C.c_int64(), C.c_int64(), C.c_int32()
    assert lib.sai_bcf_stitch(ptr(chains), ptr(info), n_bytes, seg_bytes, max_heads, e0, ptr(seg_entry), ptr(seg_first), C.byref(n_records),
                              C.byref(carry_from), C.byref(verdict)) == 0, lib.sai_last_error()  # fmt: skip
    got = dict(data=data, chains=chains, info=info, seg_entry=seg_entry, seg_first=seg_first, n_records=int(n_records.value),
               carry_from=int(carry_from.value), verdict=int(verdict.value), heads=None)  # fmt: skip
    if not got["verdict"]:
        got["heads"] = heads_of(data, n_bytes, seg_bytes, seg_entry, seg_first, got["carry_from"], got["n_records"], st.gt_key, want_gt)
    return got


def assert_heads_are(heads, records, where=""):
    assert len(heads) == len(records), where
    for h, r in zip(heads, records):
        assert (int(h["off"]), int(h["l_shared"]), int(h["l_indiv"]), int(h["chrom"]), int(h["pos0"]), int(h["n_allele"]), int(h["n_fmt"])) == (
            r["off"], r["l_shared"], r["l_indiv"], r["chrom"], r["pos0"], r["n_allele"], r["n_fmt"]), (where, r)  # fmt: skip
        assert (int(h["ref_len"]), h["ref"], int(h["alt_len"]), h["alt"]) == (min(len(r["ref"]), 255), r["ref"][:12], min(len(r["alt"]), 255), r["alt"][:12]), (where, r)
        assert int(h["flags"]) == 0 and (int(h["gt_off"]), int(h["gt_width"]), int(h["gt_len"])) == r["gt"], (where, r)


def assert_clean_walk(st, seg_bytes, where=""):
    """The whole stream as one batch gives exactly the builder's records, and no segment is dense."""
    got = walk(st, seg_bytes)
    assert not (got["info"] & DENSE).any(), (where, seg_bytes)
    assert got["verdict"] == 0 and got["n_records"] == len(st.records) and got["carry_from"] == len(st.bytes), (where, seg_bytes)
    assert_heads_are(got["heads"], st.records, (where, seg_bytes))
    return got


SHAPES = [dict(width=1), dict(width=2, extra_before=True), dict(width=4, extra_after=True), dict(width=1, idx=True, extra_before=True, extra_after=True),
          dict(width=2, idx=True)]  # fmt: skip


def one_sample_vcf(n_records=40, id_of=lambda k: f"v{k}", samples=("a",), chroms=("5",)) -> str:
    lines = ["##fileformat=VCFv4.2"] + [f"##contig=<ID={c}>" for c in chroms] + ['##FORMAT=<ID=GT,Number=1,Type=String,Description="g">',
             "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples)]  # fmt: skip
    for k in range(n_records):
        calls = "\t".join(["0|1", "1/1", "0|0"][(k + j) % 3] for j in range(len(samples)))
        lines.append(f"{chroms[k * len(chroms) // n_records]}\t{100 + 3 * k}\t{id_of(k) or '.'}\tA\tC\t.\t.\t.\tGT\t{calls}")
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("seg_bytes", [256, 1024, 65536])
def test_the_walk_returns_the_builders_records(seg_bytes):
    """Offsets, fixed fields, alleles and the GT location for every shape the builder writes."""
    for name in ("example.vcf", "seeded"):
        for shape in SHAPES:
            assert_clean_walk(Stream(vcf_text(name), **shape), seg_bytes, (name, shape))


def test_a_record_start_at_every_position_relative_to_a_segment_boundary():
    """The length of record 3's ID moves the start of record 4 through the 32 positions at which its fixed fields
    split k / 32 - k over a boundary (k = 0: it starts at the boundary)."""
    seen = set()
    for pad in range(0, 300):
        st = Stream(one_sample_vcf(12, id_of=lambda k: "x" * pad if k == 3 else ""))
        k = -st.records[4]["off"] % 256
        if k < 32 and k not in seen:
            seen.add(k)
            got = assert_clean_walk(st, 256, k)
            assert got["seg_entry"][st.records[4]["off"] // 256 + (k > 0)] >= 0
        if len(seen) == 32:
            break
    assert seen == set(range(32))


def test_long_and_short_records():
    """A record longer than five segments of 256 bytes, and one-sample records of about 45 bytes, five or more to a segment."""
    st = Stream(one_sample_vcf(9, samples=[f"s{k}" for k in range(700)]))
    assert all(r["l_shared"] + r["l_indiv"] + 8 > 5 * 256 for r in st.records)
    for seg_bytes in (256, 16384):
        assert_clean_walk(st, seg_bytes)
    st = Stream(one_sample_vcf(60))
    sizes = [8 + r["l_shared"] + r["l_indiv"] for r in st.records]
    assert 40 <= min(sizes) and max(sizes) <= 50
    got = assert_clean_walk(st, 256)
    assert int(got["chains"]["n_records"].max()) >= 5


def decoy_stream(n_copies=3, gap=0, align=0, last=False):
    """One-sample records; every record from the fourth on carries, in a char FORMAT field (in front of GT, or behind
    it: ``last``), ``align`` bytes and then ``n_copies`` byte copies of complete real records, ``gap`` bytes between them."""
    plain = Stream(one_sample_vcf(30))
    real = [plain.bytes[r["off"] : r["off"] + 8 + r["l_shared"] + r["l_indiv"]] for r in plain.records]

    def hook(i, rec):
        if i >= 3:
            payload = b"\x07" * align + (b"\x07" * gap).join(real[(i + j) % 3] for j in range(n_copies)) + b"\x07" * gap
            field = {"key": 0, "type": B.CHAR, "L": len(payload), "payload": payload}
            rec["fmt"] = rec["fmt"] + [field] if last else [field] + rec["fmt"]

    return plain, Stream(one_sample_vcf(30), on_record=hook)


def test_decoys_add_heads_and_change_nothing():
    plain, _ = decoy_stream()
    base = int((walk(plain, 256)["info"] & 0xFFFF).sum())
    for align in (0, 1, 2, 3, 5, 16, 31):
        _, st = decoy_stream(align=align)
        got = assert_clean_walk(st, 256, align)
        assert int((got["info"] & 0xFFFF).sum()) > base + 20
        assert_clean_walk(st, 1024, align)
    # behind GT the last copy's successor is the next true record: still the builder's chain wherever the stitch follows it
    _, st = decoy_stream(last=True)
    got = walk(st, 1024)
    assert got["verdict"] == 1 or (got["n_records"] == len(st.records) and [int(h["off"]) for h in got["heads"]] == [r["off"] for r in st.records])


def test_more_decoys_than_max_heads_give_the_host_route():
    """Ten copies with a byte between them are ten heads in one segment of 1 024 bytes: dense, and the verdict is the host route."""
    _, st = decoy_stream(n_copies=10, gap=1)
    got = walk(st, 1024)
    assert (got["info"] & DENSE).any() and got["verdict"] == 1 and got["heads"] is None
    assert_clean_walk(st, 256)  # at most six copies start in a segment of 256 bytes, next to the true record
    got = walk(st, 1024, max_heads=64)
    assert got["verdict"] == 0 and [int(h["off"]) for h in got["heads"]] == [r["off"] for r in st.records]


@pytest.mark.parametrize("damage", [dict(l_indiv=77), dict(n_sample=10), dict(chrom=5)])
def test_a_broken_chain_gives_the_host_route(damage):
    for seg_bytes in (256, 65536):
        st = Stream(vcf_text("example.vcf"), on_record=lambda i, r: i == 6 and r.update(damage))
        got = walk(st, seg_bytes)
        assert got["verdict"] == 1 and got["n_records"] <= 7, (damage, seg_bytes)


def test_an_incomplete_last_record_is_carried():
    st = Stream(vcf_text("example.vcf"), width=2)
    for cut_in in (5, 12):
        for inside in (1, 7, 8, 31, 32, 40):
            cut = st.records[cut_in]["off"] + inside
            for seg_bytes in (256, 16384):
                first = walk(st, seg_bytes, data=st.bytes[:cut])
                assert first["verdict"] == 0 and first["carry_from"] == st.records[cut_in]["off"] and first["n_records"] == cut_in, (cut_in, inside)
                assert_heads_are(first["heads"], st.records[:cut_in])
                rest = walk(st, seg_bytes, data=st.bytes[first["carry_from"] :], e0=0)
                assert rest["verdict"] == 0 and rest["n_records"] == len(st.records) - cut_in and rest["carry_from"] == len(st.bytes) - first["carry_from"]
                shifted = [dict(r, off=r["off"] - first["carry_from"], gt=(r["gt"][0] - first["carry_from"],) + r["gt"][1:]) for r in st.records[cut_in:]]
                assert_heads_are(rest["heads"], shifted)
    empty = walk(st, 256, data=st.bytes[: st.data_off])  # nothing behind the header
    assert empty["verdict"] == 0 and empty["n_records"] == 0 and empty["carry_from"] == st.data_off


class Feed:
    def __init__(self, path, chrom, samples=(), start=None, end=None, anc=None, text_batch=1 << 20, whole_file=False, comp_cap=1 << 18):
        from sai_amd import _ffi_bcf_device as D

        self.lib, self.D = D.load_host(), D
        self.bufs = [np.zeros(comp_cap, dtype=np.uint8) for _ in range(2)]
        self.handle = C.c_void_p()
        names = (C.c_char_p * len(samples))(*[s.encode() for s in samples])
        self.rc = self.lib.sai_bcf_feed_open(str(path).encode(), chrom.encode(), -1 if start is None else start, -1 if end is None else end, len(samples),
                                             names, anc.encode() if anc else None, ptr(self.bufs[0]), ptr(self.bufs[1]), comp_cap, text_batch,
                                             int(whole_file), C.byref(self.handle))  # fmt: skip

    def close(self):
        self.lib.sai_bcf_feed_close(self.handle)

    def batches(self):
        """(inflated text of the batch, e0) per batch, the members inflated here with zlib and checked against their CRC."""
        while True:
            b, n_comp, nm, n_text, e0, done = C.c_int32(), C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int32()
            members = C.c_void_p()
            assert self.lib.sai_bcf_feed_next(self.handle, *[C.byref(x) for x in (b, n_comp, nm, members, n_text, e0, done)]) == 0
            if done.value:
                return
            table = np.ctypeslib.as_array(C.cast(members, C.POINTER(C.c_uint8)), shape=(nm.value * 32,)).copy()
            comp, out = self.bufs[b.value].tobytes(), bytearray(n_text.value)
            assert n_comp.value % 4 == 0
            for m in range(nm.value):
                data_off, out_off, data_len, isize, crc, _ = struct.unpack_from("<qqIIII", table, 32 * m)
                piece = zlib.decompress(comp[data_off : data_off + data_len], -15)
                assert len(piece) == isize and zlib.crc32(piece) == crc
                out[out_off : out_off + isize] = piece
            yield bytes(out), e0.value

    def select(self, heads):
        n_rows, done, verdict = C.c_int64(), C.c_int32(), C.c_int32()
        tabs = [C.c_void_p() for _ in range(5)]
        assert self.lib.sai_bcf_feed_select(self.handle, ptr(heads), len(heads), C.byref(n_rows), *[C.byref(t) for t in tabs], C.byref(done), C.byref(verdict)) == 0
        kinds = (C.c_int32, C.c_uint8, C.c_int64, C.c_uint8, C.c_int32)
        cols = [np.ctypeslib.as_array(C.cast(t, C.POINTER(ct)), shape=(n_rows.value,)).copy() if n_rows.value else np.zeros(0, dtype=np.int64)
                for t, ct in zip(tabs, kinds)]  # fmt: skip
        return cols, bool(done.value), verdict.value

    def counts(self):
        v = [C.c_int64() for _ in range(5)]
        assert self.lib.sai_bcf_feed_selection(self.handle, None, 0, None, 0, None, None, None, *[C.byref(x) for x in v]) == 0
        return tuple(x.value for x in v)


def test_the_feed_hands_the_members_over(tmp_path):
    """Small members and a small batch: the batches, inflated, are the stream from the member in which the header ends, and
    e0 of the first is the first byte behind the header."""
    for name, shape in (("example.vcf", dict(member_size=300)), ("example.vcf", dict(member_size=200, eof=False, width=2)), ("seeded", dict(member_size=977))):
        st = Stream(vcf_text(name), **{k: v for k, v in shape.items() if k not in ("member_size", "eof")})
        path = B.write_bcf(tmp_path / "f.bcf", vcf_text(name), **shape)
        for text_batch in (700, 4096, 1 << 20):
            feed = Feed(path, "21", text_batch=text_batch)
            assert feed.rc == 0
            got = list(feed.batches())
            feed.close()
            first = st.data_off // shape["member_size"] * shape["member_size"]  # the members are cut every member_size bytes
            assert got[0][1] == st.data_off - first and all(e0 == 0 for _, e0 in got[1:])
            assert b"".join(t for t, _ in got) == st.bytes[first:]
            assert all(len(t) <= max(text_batch, shape["member_size"]) for t, _ in got) and (text_batch > 700 or len(got) > 1)


@pytest.mark.parametrize("name,chrom,given_anc", FILES, ids=[f[0] for f in FILES])
def test_feed_select_equals_the_host_stream(tmp_path, name, chrom, given_anc):
    """pos, flip, width, L and the GT bytes row for row, n_matched and n_anc: whole chromosome and region, with and without
    ancestral alleles, the stream walked in batches with the carry in front (the early stop included)."""
    from sai_amd import _ffi_bcf
    from sai_amd.utils import bcf

    samples = samples_of(name)
    anc, region = anc_file(name, chrom, given_anc, tmp_path), region_of(name, chrom)
    seg_bytes = 256 if len(samples) < 100 else 16384
    for k, shape in enumerate((dict(width=1, member_size=300), dict(width=2, idx=True, extra_before=True, extra_after=True, member_size=977, eof=False))):
        path = B.write_bcf(tmp_path / f"{k}.bcf", vcf_text(name), **shape)
        st = Stream(vcf_text(name), **{k: v for k, v in shape.items() if k not in ("member_size", "eof")})
        for a, (start, end) in ((None, (None, None)), (anc, (None, None)), (None, region), (anc, region)):
            cap = 1 << 22
            bufs = [np.zeros(cap, dtype=np.uint8) for _ in range(2)]
            want_rows = []
            with bcf._Stream(_ffi_bcf.load_host(), path, chrom, samples[:2], [2, 2], start, end, a, 2, [b.ctypes.data for b in bufs], cap) as host:
                while (got := host.next()) is not None:
                    b, _, pos, flip, off, width, length = got
                    for r in range(len(pos)):
                        n = len(samples) * int(width[r]) * int(length[r])
                        want_rows.append((int(pos[r]), int(flip[r]), int(width[r]), int(length[r]), bufs[b][off[r] : off[r] + n].tobytes()))
                want_counts = host.counts()
            feed = Feed(path, chrom, samples[:2], start, end, a, text_batch=max(700, 12 * len(samples)))
            assert feed.rc == 0
            rows, carry, stopped, n_batches = [], b"", False, 0
            for text, e0 in feed.batches():
                data = carry + text
                got = walk(st, seg_bytes, data=data, e0=0 if carry else e0)
                assert got["verdict"] == 0 and not (got["info"] & DENSE).any()
                (pos, flip, off, width, length), stopped, verdict = feed.select(got["heads"])
                assert verdict == 0
                for r in range(len(pos)):
                    n = len(samples) * int(width[r]) * int(length[r])
                    rows.append((int(pos[r]), int(flip[r]), int(width[r]), int(length[r]), data[off[r] : off[r] + n]))
                carry, n_batches = data[got["carry_from"] :], n_batches + 1
                if stopped:
                    break
            assert (stopped or not carry) and n_batches > 1
            assert rows == want_rows and feed.counts()[:2] == want_counts, (name, shape, a, start)
            feed.close()
        # the scan: every record counted, first and last of the run
        feed = Feed(path, chrom, whole_file=True)
        heads = walk(st, seg_bytes, want_gt=False)["heads"]
        _, stopped, verdict = feed.select(heads)
        assert not stopped and verdict == 0 and feed.counts()[2:] == (len(st.records), *bcf.scan_first_last(path, chrom))
        feed.close()


def test_what_open_and_select_hand_to_the_host_route(tmp_path):
    from sai_amd import _ffi_bcf_device as D

    samples = samples_of("example.vcf")
    path = small_bcf(tmp_path)
    long_anc = tmp_path / "long.bed"
    pos = int(vcf_text("example.vcf").split("\n")[-2].split("\t")[1])
    long_anc.write_text(f"21\t{pos - 1}\t{pos}\tACGTACGTACGTA\n")  # 13 bytes: a head carries 12
    for anc, rc in ((str(long_anc), D.SAI_BCF_HOST_ROUTE), (None, 0)):
        feed = Feed(path, "21", samples, anc=anc)
        assert feed.rc == rc
        if rc == 0:
            feed.close()
    feed = Feed(path, "21", ["nobody"])
    assert feed.rc == D.SAI_BCF_HOST_ROUTE
    # a GT vector that says three values per sample and holds two: the chain is whole, the array leaves the record
    cases = [(n, o) for n, o, _ in REFUSED] + [("gt_longer", dict(on_record=lambda i, r: i == 3 and _gt(r).update(L=3)))]
    for name, options in cases:
        if name in ("no_gt_entry", "typed_value_leaves", "gt_leaves", "gt_float", "gt_char", "no_gt_key", "gt_longer"):
            damaged = small_bcf(tmp_path, name + ".bcf", **options)
            st = Stream(vcf_text("example.vcf"), **{k: v for k, v in options.items() if k == "on_record"})
            if name == "no_gt_key":
                st.gt_key = -1
            got = walk(st, 256)
            if name in ("typed_value_leaves", "gt_leaves"):
                assert got["verdict"] == D.SAI_BCF_HOST_ROUTE, name  # a wrong l_indiv breaks the chain itself
                continue
            assert got["verdict"] == 0, name  # the chain is whole: it is the selection that meets the flag
            feed = Feed(damaged, "21", samples)
            assert feed.rc == 0 and feed.select(got["heads"])[2] == D.SAI_BCF_HOST_ROUTE, name
            feed.close()
            feed = Feed(damaged, "21")  # no genotypes asked for: nothing of the individual part is looked at
            assert feed.rc == 0 and feed.select(walk(st, 256, want_gt=False)["heads"])[2] == 0, name
            feed.close()


@pytest.fixture(scope="module")
def walk_dump_programs(tmp_path_factory):
    """tests/native/bcf_walk_dump.cpp + the host units of libsaihip, once under ASan + UBSan with the runtimes linked in
    (as test_bcf_cpu.py::dump_programs builds its program) and once plain."""
    return native_build.dump_program("bcf_walk_dump", tmp_path_factory, kinds=("san", "plain"))


def run_walk_dump(exe, path, chrom, start, end, anc, seg_bytes, text_batch, whole_file, samples):
    return native_build.run_native(exe, [path, chrom, -1 if start is None else start, -1 if end is None else end, anc or "-", seg_bytes, MAX_HEADS,
                                         text_batch, int(whole_file), *samples])  # fmt: skip


def test_host_code_is_clean_under_asan_ubsan(tmp_path, walk_dump_programs):
    """The feed, the twins, the stitch and the selection, run (not only compiled) under the sanitizers in the loop of the
    reader: the files above, the decoy files and every damaged file.  Clean, the same output as the plain build, the
    rows of the host reader."""
    from sai_amd.utils import bcf

    def both(*args):
        got = {kind: run_walk_dump(exe, *args) for kind, exe in walk_dump_programs.items()}
        assert got["san"].returncode in (0, 4), got["san"].stderr[-3000:]
        assert (got["san"].stdout, got["san"].returncode) == (got["plain"].stdout, got["plain"].returncode) and not got["san"].stderr
        return got["san"]

    runs = 0
    for k, (name, chrom, given_anc) in enumerate(FILES):
        samples = samples_of(name)
        path = B.write_bcf(tmp_path / f"f{k}.bcf", vcf_text(name), **[dict(width=1, member_size=300), dict(width=2, idx=True, extra_before=True, member_size=977, eof=False)][k % 2])
        anc, region = anc_file(name, chrom, given_anc, tmp_path), region_of(name, chrom)
        for a, (start, end) in ((None, (None, None)), (anc, region)):
            res = both(path, chrom, start, end, a, 256 if len(samples) < 100 else 4096, max(3000, 12 * len(samples)), 0, samples[:3])
            assert res.returncode == 0 and "verdict 1" not in res.stdout
            want = bcf.load_dosage(path, chrom, samples[:3], [2, 2, 2], start, end, a)
            rows = [ln.split() for ln in res.stdout.split("\n") if re.match(r"^\d", ln)]
            assert [int(r[0]) for r in rows] == want[0].tolist()
            assert re.search(rf"^counts {want[2]} {want[3]} ", res.stdout, re.M)
            runs += 1
        res = both(path, chrom, None, None, None, 1024, 5000, 1, [])
        first, last = bcf.scan_first_last(path, chrom)
        assert re.search(rf"^counts \d+ 0 records {bcf.header_counts(path)[0]} first {first} last {last}$", res.stdout, re.M)
        runs += 1
    for n_copies, gap, want_rc in ((3, 0, 0), (10, 1, 4)):
        _, st = decoy_stream(n_copies=n_copies, gap=gap)
        path = tmp_path / f"decoy{n_copies}.bcf"
        path.write_bytes(b"".join(B.bgzf_members(st.bytes, member_size=900)))
        res = both(path, "5", None, None, None, 1024, 2500, 0, ["a"])
        assert res.returncode == want_rc and (want_rc == 0 or "host-route stitch" in res.stdout)
        if want_rc == 0:
            assert [int(ln.split()[0]) for ln in res.stdout.split("\n") if re.match(r"^\d", ln)] == [r["pos0"] + 1 for r in st.records]
        runs += 1
    samples = samples_of("example.vcf")
    for name, options, _ in REFUSED:
        if name == "raw":
            continue
        res = both(small_bcf(tmp_path, name + ".bcf", **options), "21", None, None, None, 256, 3000, 0, samples)
        assert res.returncode == 4 and re.search(r"^host-route \S+$", res.stdout, re.M), (name, res.stdout[-500:])
        runs += 1
    # A member whose XLEN (file content) claims more than a member can hold, starting where the program's buffers of
    # 131 136 bytes have just room for one member more (at most 65 596 bytes are filled): it is refused before anything
    # behind its first 12 bytes is read, where reading XLEN bytes would end past the caller's buffer (exit status 6: the
    # program keeps guard bytes behind its buffers, since the sanitizers do not see what fread writes).
    st = Stream(vcf_text("example.vcf"))
    good = B.bgzf_members(st.bytes, member_size=300)
    padded = lambda m: len(m) + -len(m) % 4  # noqa: E731
    filled = sum(padded(m) for m in good[st.data_off // 300 :])  # the first batch starts at the member in which the header ends

    def filler(size):
        """An empty BGZF member of `size` bytes (a multiple of 4): a second extra subfield takes the room."""
        extra = b"BC\x02\x00" + struct.pack("<H", size - 1) + b"XX" + struct.pack("<H", size - 32) + bytes(size - 32)
        return b"\x1f\x8b\x08\x04" + bytes(6) + struct.pack("<H", len(extra)) + extra + b"\x03\x00" + bytes(8)

    for xlen, fill_to in ((65535, 65596), (65529, 65596), (65528, 65592)):
        path = tmp_path / f"xlen{xlen}.bcf"
        rest = fill_to - filled
        fillers = [filler(rest - 40000), filler(40000)] if rest > 60000 else [filler(rest)]
        assert filled + sum(len(f) for f in fillers) == fill_to and all(len(f) % 4 == 0 for f in fillers)
        path.write_bytes(b"".join(good + fillers) + b"\x1f\x8b\x08\x04" + bytes(6) + struct.pack("<H", xlen) + b"BC\x02\x00" + bytes(xlen))
        res = both(path, "21", None, None, None, 256, 1 << 20, 0, samples)
        assert res.returncode == 4 and "host-route reader" in res.stdout, (xlen, res.stdout[-300:])
        runs += 1
    assert runs == 3 * len(FILES) + 2 + len(REFUSED) - 1 + 3


def test_header_binding_and_library_agree():
    from sai_amd import _build, _ffi_bcf, _ffi_bcf_device as D

    names = abi_checks.declared_names("saihip_bcf_device.h")
    assert names == sorted(D.SIGNATURES) and len(names) == 13
    lib = D.load()
    version = abi_checks.header_macro("saihip_bcf_device.h", "SAI_BCF_DEVICE_ABI_VERSION")
    assert lib.sai_bcf_device_abi_version() == D.SAI_BCF_DEVICE_ABI_VERSION == version == 1
    macros = re.findall(r"#define (SAI_BCF_[A-Z_]+) \d+", abi_checks.header_text("saihip_bcf_device.h"))
    assert len(macros) == 13
    for name in macros:
        assert abi_checks.header_macro("saihip_bcf_device.h", name) == getattr(D, name), name
    assert len(abi_checks.declared_names("saihip_bcf.h")) == len(_ffi_bcf.SIGNATURES) == 10
    assert "bcf/bcf_walk.hip" in _build.UNITS and "bcf/bcf_feed.cpp" in _build.HOST_UNITS
    assert ROOT / "include" / "saihip_bcf_device.h" in _build.PUBLIC_HEADERS and "csrc/bcf/*.hpp" in abi_checks.package_data_patterns()
    assert _build.CSRC / "bcf" / "bcf_record.hpp" in _build.staleness_inputs()
    assert lib.sai_bcf_chain_segments(None, None, 0, 256, 8, None, 0, 0, None, None, None) != 0 and b"ctx is NULL" in lib.sai_last_error()
