"""sai_inflate_bgzf on streams that zlib's encoder never writes: hand-built DEFLATE members from
tests/deflate_builder.py (proven against zlib's decoder in test_deflate_builder_cpu.py), on every
instantiation of the kernel (SAI_INFLATE_WINDOW), with the boundary between the LDS history and the
HBM read-back hit from both sides, every invalid class the kernel has a branch for, the CRC kernel
at its slice edges, the product route on a file from this encoder, and libdeflate's encoder where
the library is there.  Every comparison is exact: bytes, status, guard bytes."""

import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import deflate_builder as db
from test_inflate_device import deflate, run, vcf_like

pytestmark = pytest.mark.gpu

GAPS = [(g, t) for g in (0, 1, 2, 3) for t in (0, 1, 5)]  # compressed-byte gaps x text gaps


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from sai_amd.engine import Engine

    return Engine.get(0)


def check_exact(eng, streams, texts, names, gap, text_gap, seed=0):
    status, outs, guards = run(eng, streams, texts, np.random.default_rng(seed), gap, text_gap)
    bad = [(names[i], int(status[i])) for i in range(len(texts)) if status[i] != 0]
    assert not bad, (gap, text_gap, bad[:10])
    wrong = [names[i] for i in range(len(texts)) if outs[i] != texts[i]]
    assert not wrong, (gap, text_gap, wrong[:10])
    assert guards, (gap, text_gap)


def run_directed(eng):
    cases = db.directed_cases()
    streams, texts, names = [c[1] for c in cases], [c[2] for c in cases], [c[0] for c in cases]
    for gap, text_gap in GAPS:
        check_exact(eng, streams, texts, names, gap, text_gap, seed=gap * 8 + text_gap)
    return len(cases) * len(GAPS)


def test_directed_streams_at_the_default_window(eng):
    """One member per case, each from explicit tokens (the list is in deflate_builder.directed_cases):
    d = W - 1, W, W + 1 for every W the kernel is built for, matches that read their own output, far
    matches at every flush phase and across the wrap of the window, the header edges, stored blocks at
    every bit offset -- at compressed-byte gaps 0-3 and text gaps 0, 1, 5."""
    assert run_directed(eng) >= 200 * 12


def test_seeded_corpus_at_the_default_window(eng):
    """300 members from random_member (a third and more of them VCF-like text through tokenize); what the
    corpus holds is asserted from its counters in test_deflate_builder_cpu.py."""
    corpus = db.seeded_corpus()
    streams, texts = [c[0] for c in corpus], [c[1] for c in corpus]
    names = ["corpus %d (%d bytes)" % (i, len(t)) for i, t in enumerate(texts)]
    for gap, text_gap in ((0, 0), (1, 3), (2, 1)):
        check_exact(eng, streams, texts, names, gap, text_gap, seed=gap)


# ---- the other three instantiations: one fresh process per value of the knob (it is read once) ----------


def _pack(blobs):
    off = np.cumsum([0] + [len(b) for b in blobs]).astype(np.int64)
    return np.frombuffer(b"".join(blobs), dtype=np.uint8), off


def _unpack(data, off):
    raw = data.tobytes()
    return [raw[off[i] : off[i + 1]] for i in range(len(off) - 1)]


def child_main(path):
    """The body of a child process: the directed members at every gap and the corpus slice, from the
    .npz the parent wrote."""
    import torch

    from sai_amd.engine import Engine

    assert torch.cuda.is_available()
    eng = Engine.get(0)
    d = np.load(path)
    n = 0
    for part, gaps in (("directed", GAPS), ("corpus", ((0, 0), (1, 3)))):
        streams, texts = _unpack(d[part + "_raw"], d[part + "_raw_off"]), _unpack(d[part + "_text"], d[part + "_text_off"])
        names = ["%s %d" % (part, i) for i in range(len(texts))]
        for gap, text_gap in gaps:
            check_exact(eng, streams, texts, names, gap, text_gap, seed=gap * 8 + text_gap)
            n += len(texts)
    print("streams ok %d" % n)


def test_every_other_window_size_and_an_unknown_one(eng, tmp_path):
    """inflate_bgzf_kernel<8192>, <16384> and <32768> (the last one without the HBM read-back) on the
    directed members and on 100 members of the corpus; a value that is none of the three is the
    default -- seen from the results alone."""
    from conftest import ROOT

    directed = db.directed_cases()
    corpus = db.seeded_corpus()
    part = [corpus[i] for i in db.WINDOW_SLICE]
    arrays = {}
    for name, raws, texts in (("directed", [c[1] for c in directed], [c[2] for c in directed]),
                              ("corpus", [c[0] for c in part], [c[1] for c in part])):  # fmt: skip
        arrays[name + "_raw"], arrays[name + "_raw_off"] = _pack(raws)
        arrays[name + "_text"], arrays[name + "_text_off"] = _pack(texts)
    f = str(tmp_path / "streams.npz")
    np.savez(f, **arrays)
    want = "streams ok %d" % (len(directed) * len(GAPS) + 2 * len(part))
    code = "import sys; sys.path[:0] = [%r, %r]\nimport test_inflate_streams_device as t\nt.child_main(sys.argv[1])\n" % (
        str(ROOT), str(ROOT / "tests"))  # fmt: skip
    for value in ("8192", "16384", "32768", "12345"):
        res = subprocess.run([sys.executable, "-c", code, f], env={**os.environ, "SAI_INFLATE_WINDOW": value},
                             capture_output=True, text=True, timeout=600)  # fmt: skip
        assert res.returncode == 0 and want in res.stdout, (value, res.stdout[-500:], res.stderr[-3000:])


# ---- invalid streams ------------------------------------------------------------------------------------


def test_every_invalid_class_is_flagged_and_its_neighbours_are_not(eng):
    """One field damaged per member (deflate_builder.invalid_cases), every member between two good
    ones: a non-zero status, the neighbours exact, every guard byte intact."""
    rng = np.random.default_rng(8)
    cases = db.invalid_cases()
    text_a = vcf_like(rng, 30000)
    good_a = deflate(text_a)
    m = db.random_member(rng, 0, 0.9, text=text_a[:9000])
    good_b, text_b = m.raw(), bytes(m.text)
    streams, texts = [good_a], [text_a]
    for k, (_, raw, text, _) in enumerate(cases):
        streams += [raw, good_b if k % 2 == 0 else good_a]
        texts += [text, text_b if k % 2 == 0 else text_a]
    status, outs, guards = run(eng, streams, texts, rng, 1, 16)
    assert guards
    for i in range(0, len(streams), 2):
        assert int(status[i]) == 0 and outs[i] == texts[i], ("neighbour", i, int(status[i]))
    for k, (name, _, text, bad) in enumerate(cases):
        got = int(status[2 * k + 1])
        if bad:
            assert got > 0, (name, got)
        else:
            assert got == 0 and outs[2 * k + 1] == text, (name, got)


# ---- the CRC kernel -------------------------------------------------------------------------------------


def test_crc_kernel_at_small_sizes_and_every_alignment(eng):
    """crc_members_kernel gives every lane a slice on the 8-byte grid of the address space; members of
    0 ... 513 bytes leave most slices empty or ragged.  Eight members of each size, laid out so that
    their outputs start at all eight residues modulo 8; then the same with one bit of the expected
    CRC flipped: every status non-zero, the text written all the same."""
    rng = np.random.default_rng(13)
    for n, members in db.crc_cases().items():
        streams, texts = [m[0] for m in members], [m[1] for m in members]
        text_gap = 1 if n % 2 == 0 else 2  # an odd stride: eight outputs in a row visit every residue
        info = {}
        status, outs, guards = run(eng, streams, texts, rng, 1, text_gap, info=info)
        residues = {(info["text_ptr"] + int(o)) % 8 for o in info["table"]["out_off"]}
        assert residues == set(range(8)), (n, residues)
        assert status.tolist() == [0] * 8 and outs == texts and guards, (n, status.tolist())
        crcs = [zlib.crc32(t) ^ (1 << int(rng.integers(32))) for t in texts]
        status, outs, guards = run(eng, streams, texts, rng, 1, text_gap, crcs=crcs)
        assert all(int(s) != 0 for s in status) and outs == texts and guards, (n, status.tolist())


# ---- the product route ----------------------------------------------------------------------------------


def test_a_bgzip_vcf_from_this_encoder_reads_like_the_host_reader(eng, tmp_path, monkeypatch):
    """A bgzip VCF whose members come from the builder -- the text cut at ragged sizes, every piece a random
    parse and a random block mix, some pure stored, some pure fixed -- through load_dosage_device (GPU
    inflate) against load_dosage (libdeflate or zlib on the host), without and with a .tbi."""
    from test_ingest_native import write_tbi, write_vcf

    from sai_amd.utils import device_vcf
    from sai_amd.utils.native_vcf import load_dosage

    rng = np.random.default_rng(21)
    plain = tmp_path / "p.vcf"
    names = write_vcf(plain, rng, 900, 45)
    text = open(plain, "rb").read()
    members = db.product_members(text, rng)
    assert len(members) > 50 and b"".join(t for _, t in members) == text
    path = tmp_path / "b.vcf.gz"
    db.write_bgzf_file(path, members)
    calls = {"n": 0}
    real = device_vcf._load_bgzf_device

    def spy(*a, **k):
        got = real(*a, **k)
        calls["n"] += got is not None
        return got

    monkeypatch.setattr(device_vcf, "_load_bgzf_device", spy)
    pick = [names[i] for i in rng.permutation(45)[:30]]
    ploidies = [int(rng.choice([1, 2, 2, 4])) for _ in pick]
    for indexed in (False, True):
        if indexed:
            write_tbi(path)
        for chrom in ("7", "21", "22"):
            pos = load_dosage(str(path), chrom, pick, ploidies, None, None, None, 2)[0]
            n = len(pos)
            assert n > 300
            for start, end in ((None, None), (int(pos[n // 5]), int(pos[3 * n // 5])), (int(pos[-50]), None), (int(pos[7]), int(pos[7]))):
                want = load_dosage(str(path), chrom, pick, ploidies, start, end, None, 2)
                for cap in (1 << 17, None):
                    before = calls["n"]
                    got = device_vcf.load_dosage_device(eng, str(path), chrom, pick, ploidies, start, end, None, 4, cap)
                    assert calls["n"] == before + 1, "the file did not take the GPU-inflate route"
                    assert got[0].tolist() == want[0].tolist() and got[2] == want[2], (indexed, chrom, start, end, cap)
                    assert np.array_equal(got[1].cpu().numpy(), want[1])


# ---- a second real encoder ------------------------------------------------------------------------------


def test_members_from_libdeflate(eng):
    """bgzip is normally linked against libdeflate: its encoder at levels 0, 1, 6, 9 and 12."""
    try:
        lib = C.CDLL("libdeflate.so.0")
        for fn in ("libdeflate_alloc_compressor", "libdeflate_deflate_compress", "libdeflate_deflate_compress_bound", "libdeflate_free_compressor"):
            getattr(lib, fn)
    except (OSError, AttributeError) as e:
        pytest.skip("libdeflate's encoder is not on this machine: %s" % e)
    lib.libdeflate_alloc_compressor.restype = C.c_void_p
    lib.libdeflate_alloc_compressor.argtypes = [C.c_int]
    lib.libdeflate_deflate_compress.restype = C.c_size_t
    lib.libdeflate_deflate_compress.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    lib.libdeflate_deflate_compress_bound.restype = C.c_size_t
    lib.libdeflate_deflate_compress_bound.argtypes = [C.c_void_p, C.c_size_t]
    lib.libdeflate_free_compressor.argtypes = [C.c_void_p]
    rng = np.random.default_rng(17)
    base = vcf_like(rng, 65536)
    streams, texts, names = [], [], []
    for level in (0, 1, 6, 9, 12):
        comp = lib.libdeflate_alloc_compressor(level)
        assert comp, level
        for n in (1, 300, 65280, 65536):
            t = base[:n]
            out = C.create_string_buffer(lib.libdeflate_deflate_compress_bound(comp, n))
            k = lib.libdeflate_deflate_compress(comp, t, n, out, len(out))
            assert k > 0
            streams.append(out.raw[:k])
            texts.append(t)
            names.append("libdeflate level %d, %d bytes" % (level, n))
            assert zlib.decompress(streams[-1], -15) == t
        lib.libdeflate_free_compressor(comp)
    for gap, text_gap in ((0, 0), (1, 1), (3, 5)):
        check_exact(eng, streams, texts, names, gap, text_gap)
