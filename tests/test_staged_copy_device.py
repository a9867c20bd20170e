"""What ``_ingest.staged_copy`` does for every device reader alike: a read that fails in the middle leaves staging the
next read can use and a drained side stream, and a buffer that is too small is refused before anything is page-locked.

One fileset in three formats: 130 variants x 400 samples, rows and records of 100 bytes, so a 4 KiB buffer takes
40 of them and the read four batches.  (At 70 samples a row is 18 bytes and the whole file one batch of 4 KiB: the
width is chosen for the number of batches.)"""

import os

import numpy as np
import pytest

import pgen_builder as B
from test_eigenstrat_cpu import eigenstrat_from_plink
from test_plink_cpu import write_fileset

pytestmark = pytest.mark.gpu

CAP = 4096
N_VARIANTS, N_SAMPLES = 130, 400
SAMPLES = [f"s{i}" for i in range(N_SAMPLES)]
POPULATIONS = [(SAMPLES[:200], 2), (SAMPLES[200:], 2)]


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from sai_amd.engine import Engine

    return Engine.get(0)


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """id -> (module, staging key, data file, host reader, device reader, their arguments), the three filesets
    written once."""
    from sai_amd.utils import eigenstrat, pgen, plink

    rng = np.random.default_rng(26)
    bed = str(tmp_path_factory.mktemp("staged") / "f")
    codes = rng.integers(0, 4, size=(N_VARIANTS, N_SAMPLES)).astype(np.uint8)
    write_fileset(bed, ["3"] * N_VARIANTS, np.cumsum(rng.integers(1, 30, N_VARIANTS)).tolist(), [f"v{k}" for k in range(N_VARIANTS)],
                  ["A"] * N_VARIANTS, ["C"] * N_VARIANTS, codes, SAMPLES)  # fmt: skip
    B.from_bed_fileset(bed, bed + "_2", [0] * N_VARIANTS)  # every record the plain 2-bit one: 100 bytes
    eigenstrat_from_plink(bed, bed + "_e", "packed")
    dosage, packed = (SAMPLES, [2] * N_SAMPLES), (POPULATIONS,)
    return {
        "bed-dosage": (plink, "_plink_state", bed + ".bed", plink.load_dosage, plink.load_dosage_device, (bed, "3", *dosage)),
        "bed-packed": (plink, "_plink_state", bed + ".bed", plink.load_packed, plink.load_packed_device, (bed, "3", *packed)),
        "pgen-dosage": (pgen, "_pgen_state", bed + "_2.pgen", pgen.load_dosage, pgen.load_dosage_device, (bed + "_2", "3", *dosage)),
        "pgen-packed": (pgen, "_pgen_state", bed + "_2.pgen", pgen.load_packed, pgen.load_packed_device, (bed + "_2", "3", *packed)),
        "geno-dosage": (eigenstrat, "_eigenstrat_state", bed + "_e.geno", eigenstrat.load_dosage, eigenstrat.load_dosage_device,
                        (bed + "_e", "3", *dosage)),
    }  # fmt: skip


ROUTES = ("bed-dosage", "bed-packed", "pgen-dosage", "pgen-packed", "geno-dosage")


def same(got, want) -> bool:
    """A device read equals the host read: positions, counts, and the dosage block or every packed block."""
    if got[0].tolist() != want[0].tolist() or got[2:] != want[2:]:
        return False
    if isinstance(want[1], list):
        return len(got[1]) == len(want[1]) and all(np.array_equal(p.data.cpu().numpy(), block) for p, block in zip(got[1], want[1]))
    return np.array_equal(got[1].cpu().numpy(), want[1])


@pytest.mark.parametrize("route", ROUTES)
def test_a_read_that_fails_in_the_middle_leaves_the_staging_usable(eng, routes, monkeypatch, route):
    module, key, data_file, host_read, device_read, args = routes[route]
    want = host_read(*args, buffer_bytes=CAP)
    assert len(want[0]) == N_VARIANTS
    # on the CPU: four batches or more, and the file ends inside the third -- both buffers have been copied from and
    # one is being reused when ``pread_into`` raises, and a batch lies behind it
    host_lib = {"_plink_state": "_ffi_plink", "_pgen_state": "_ffi_pgen", "_eigenstrat_state": "_ffi_eigenstrat"}[key]
    idx = module._Index(getattr(module, host_lib).load_host(), args[0], "3", SAMPLES, [2] * N_SAMPLES, None, None, None, 2)
    batches = list(idx.staged(CAP))
    assert len(batches) >= 4
    _, file_offset, n = batches[2][0][-1]
    cut = file_offset + n // 2
    assert all(off + m <= cut for reads, _, _ in batches[:2] for _, off, m in reads) and cut < min(off for _, off, _ in batches[3][0])
    intact = open(data_file, "rb").read()
    real_index = module._Index

    def index_then_truncate(*a, **kw):  # the index checks the size of the file: it ends early only once the index is built
        built_index = real_index(*a, **kw)
        os.truncate(data_file, cut)
        return built_index

    module.release_buffers(eng)
    try:
        with monkeypatch.context() as patch:
            patch.setattr(module, "_Index", index_then_truncate)
            with pytest.raises(ValueError, match=rf"{os.path.basename(data_file)}: read error or unexpected end of file at byte \d+"):
                device_read(eng, *args, buffer_bytes=CAP)
    finally:
        with open(data_file, "wb") as f:
            f.write(intact)
    staging = eng.__dict__[key]
    pinned = [t.data_ptr() for t in staging["pinned"]]
    assert staging["cap"] == CAP and staging["stream"].query()  # the side stream is drained
    got = device_read(eng, *args, buffer_bytes=CAP)
    assert same(got, want)
    assert eng.__dict__[key] is staging and [t.data_ptr() for t in staging["pinned"]] == pinned  # ... and the staging reused


@pytest.mark.parametrize("route", ROUTES)
def test_a_buffer_below_one_row_is_refused_before_anything_is_page_locked(eng, routes, route):
    module, key, data_file, _, device_read, args = routes[route]
    what = "record" if key == "_pgen_state" else "row"
    module.release_buffers(eng)
    assert key not in eng.__dict__
    with pytest.raises(ValueError, match=rf"SAI_AMD_INGEST_BUFFER of 99 bytes is smaller than one {what} of .*{os.path.basename(data_file)} \(100 bytes"):
        device_read(eng, *args, buffer_bytes=99)
    assert key not in eng.__dict__
    assert same(device_read(eng, *args, buffer_bytes=CAP), routes[route][3](*args, buffer_bytes=CAP))
