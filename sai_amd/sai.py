"""``score`` and ``outlier`` -- the functions behind ``sai score`` / ``sai outlier`` (mirror of
sai/sai.py:33-230)."""

from __future__ import annotations

import os
import warnings
from pathlib import Path

import yaml

from .configs import GlobalConfig
from .generators import ChunkGenerator
from .preprocessors import ChunkPreprocessor
from .utils import UniqueKeyLoader

_POLARISED = ("fd", "df", "Danc", "Dplus")


def load_config(config: str) -> GlobalConfig:
    """YAML -> GlobalConfig with the reference's error behaviour (sai.py:65-73)."""
    try:
        with open(config, "r") as f:
            config_dict = yaml.load(f, Loader=UniqueKeyLoader)
    except FileNotFoundError:
        raise FileNotFoundError(f"Configuration file '{config}' not found.")
    except yaml.YAMLError as e:
        raise ValueError(f"Error parsing YAML configuration file '{config}': {e}")
    return GlobalConfig(**config_dict)


def header_line(stat_config, ploidy_config) -> str:
    """sai.py:107-131: fixed columns + one column per statistic in YAML order (U/Q always a
    single column; a statistic set to False is left out)."""
    cols = ["Chrom", "Start", "End", "Ref", "Tgt", "Src", "Outgroup", "N(Variants)"]
    src_pops = list(ploidy_config.root["src"].keys())
    for name, value in stat_config.root.items():
        if name not in ("U", "Q") and value is False:
            continue
        if name in ("U", "Q") or len(src_pops) <= 1:
            cols.append(name)
        else:
            cols.extend(f"{name}.{sp}" for sp in src_pops)
    return "\t".join(cols) + "\n"


def write_headers(output_file: str, stat_config, ploidy_config) -> None:
    """Create the output directory, the TSV with its header and the .U.log/.Q.log files
    (sai.py:133-144)."""
    directory = os.path.dirname(output_file)
    if directory:
        os.makedirs(directory, exist_ok=True)
    with open(output_file, "w") as f:
        f.write(header_line(stat_config, ploidy_config))
    for key in ("U", "Q"):
        if key in stat_config.root:
            with open(Path(output_file).with_suffix(f".{key}.log"), "w") as f:
                f.write(f"Chrom\tStart\tEnd\t{key}_SNP\n")


def require_polarised_input(stat_config, anc_allele_file) -> None:
    """fd, df, Danc and Dplus need polarised data (sai.py:79-84)."""
    if anc_allele_file is not None:
        return
    wanted = [name for name in stat_config.root if name in _POLARISED]
    if wanted:
        raise ValueError(
            f"The {wanted[0]} statistic requires polarized data, please provide the ancestral allele information with `--anc-alleles`."
        )


def chunk_preprocessor_for(cfg: GlobalConfig, vcf_file, win_len, win_step, output_file, anc_allele_file,
                           layout: str = "int8", src_file=None) -> ChunkPreprocessor:
    """The chunk driver of a run: the sample lists come from the configuration's ``populations``
    section (sai.py:95-107).  Shared by ``score`` and ``sai_amd.distributed.score_sharded``.  ``src_file``: the
    samples of the ``src`` list are read from that file (``require_second_input``)."""
    files = {group: cfg.populations.get_population(group) for group in ("ref", "tgt", "src", "outgroup")}
    second = {} if src_file is None else {"src_file": src_file}
    return ChunkPreprocessor(vcf_file, files["ref"], files["tgt"], files["src"], files["outgroup"], win_len, win_step,
                             output_file, cfg.ploidies, cfg.statistics, anc_allele_file=anc_allele_file, layout=layout, **second)  # fmt: skip


LAYOUTS = ("int8", "packed2")


def resolve_layout(layout=None) -> str:
    """The genotype layout of a run: the argument, else ``SAI_AMD_LAYOUT``, else ``int8``."""
    layout = layout or os.environ.get("SAI_AMD_LAYOUT") or "int8"
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {', '.join(LAYOUTS)}, not {layout!r}.")
    return layout


def require_packed2_input(vcf_file, config: str, num_workers: int) -> None:
    """What ``layout="packed2"`` cannot serve is refused here, before any genotype is read: the layout is decoded
    from PLINK 1 ``.bed`` rows or PLINK 2 ``.pgen`` records on the GPU of one process and feeds the U / Q site pass
    and the frequency pass of fd, df, Danc and Dplus (``sai_amd.packed_stats``); DD has no form in it.
    (The sentences about the input and about the statistics predate the ``.pgen`` and the ABBA-BABA family in this
    layout: they are pinned word for word, and still name PLINK 1 and U / Q only.)"""
    from . import launcher
    from .utils import pgen, plink
    from .utils.filesets import reader_for

    if num_workers > 1 or launcher.in_rank_job():
        raise ValueError("layout 'packed2' runs in one process on one GPU: use num_workers=1 outside a rank job, or layout 'int8'.")
    if os.environ.get("SAI_AMD_INGEST", "device") == "host":
        raise ValueError("layout 'packed2' is decoded on the GPU: it cannot be combined with SAI_AMD_INGEST=host.")
    if reader_for(vcf_file) not in (plink, pgen):
        raise ValueError(f"layout 'packed2' reads a PLINK 1 fileset (.bed + .bim + .fam) only, which {vcf_file} is not.")
    stats = load_config(config).statistics.root
    other = [name for name, value in stats.items() if name not in ("U", "Q", *_POLARISED) and value is not False]
    if other:
        raise ValueError(f"layout 'packed2' serves the U and Q statistics only, but {other[0]} is configured.")


def require_second_input(vcf_file, src_file, anc_allele_file, layout: str) -> None:
    """What ``score(..., src_file=)`` cannot serve is refused here, before anything is read or written: two inputs are
    reconciled through the ancestral allele (``site_join.require_second_input``, whose sentence this raises), they are
    read in the int8 layout, and the file has to exist as the main input has to."""
    from . import site_join
    from .utils.filesets import is_fileset

    from .site_join_many import as_list

    files = as_list(src_file)  # one path, or the 2 to 16 of several source files: every refusal applies to every file
    site_join.require_second_input(files[0], anc_allele_file)
    if layout == "packed2":
        raise ValueError("a source file of its own is read in the int8 layout: `src_file` cannot be combined with layout 'packed2'.")
    for f in files:
        if not is_fileset(f) and not os.path.exists(f):
            raise ValueError(f"cannot open VCF {f}")  # the words a missing main input is refused with


def _reads_in_one_pass(vcf_file: str) -> bool:
    """A plain-text VCF on a machine with a GPU: the chromosome's first and last position (a host scan of
    the file, chunk_generator.py:64-82) are found WHILE the one streaming read fills HBM -- the scan was 10
    of the 24 ms of a 482 MB file.  Compressed files keep the order scan, then read: an indexed one scans
    two records, and the scan of an unindexed bgzip file is itself a pass of the GPU reader.  A PLINK fileset is
    scanned from its ``.bim`` alone (an EIGENSOFT one from its ``.snp``), which the read would index a second time:
    scan, then read."""
    from .utils.filesets import is_fileset

    if is_fileset(vcf_file):
        return False
    if str(vcf_file).endswith((".gz", ".bgz")) or os.environ.get("SAI_AMD_INGEST", "device") == "host":
        return False
    if os.environ.get("SAI_AMD_ONE_PASS", "1") == "0" or not os.path.isfile(vcf_file):
        return False
    try:
        import torch

        return bool(torch.cuda.is_available())
    except ImportError:
        return False


def _is_device_failure(exc: BaseException) -> bool:
    """A HIP call, the device or its memory failed -- anywhere in the exception's chain (the readers wrap what
    they meet in the reference's ``ValueError("Failed to read VCF file ...")``, utils.py:139-140)."""
    from . import _ffi

    seen = set()
    while exc is not None and id(exc) not in seen:
        seen.add(id(exc))
        if isinstance(exc, _ffi.SaiHipError) and exc.status in (_ffi.SAI_ERR_HIP, _ffi.SAI_ERR_NO_DEVICE):
            return True
        if isinstance(exc, MemoryError) or type(exc).__name__ in ("OutOfMemoryError", "AcceleratorError"):
            return True
        if isinstance(exc, RuntimeError) and not isinstance(exc, _ffi.SaiHipError) and ("HIP error" in str(exc) or "hip" in str(exc)[:200].lower()):
            return True
        exc = exc.__cause__ or exc.__context__
    return False


def _scan_while_reading(driver: ChunkPreprocessor, vcf_file: str, chr_name: str):
    """((first, last) of the scan, what ``ChunkPreprocessor.preload`` read meanwhile or None).  The scan's
    answer decides: a chromosome it does not find is reported as ``ChunkGenerator`` reports it, and a
    read that failed over the FILE (a malformed line, an unknown sample, no ancestral allele ...) is left to be
    repeated -- and to fail with its own message -- in the usual order.  A failure of the device is not: it is
    raised here, by the call that met it, not after a second full read."""
    from concurrent.futures import ThreadPoolExecutor

    from .utils.native_vcf import scan_first_last

    with ThreadPoolExecutor(1) as pool:
        scan = pool.submit(scan_first_last, vcf_file, chr_name)  # host threads inside libsaihip; the GIL is released
        try:
            preloaded = driver.preload(chr_name)
        except Exception as exc:  # noqa: BLE001 -- a file-level error: repeated by run_compact without the preload
            if _is_device_failure(exc):
                scan.result()
                raise
            preloaded = None
        span = scan.result()
    return span, preloaded


def chunks_for_memory(vcf_file: str, layout: str = "int8", src_file=None) -> int:
    """How many ChunkGenerator chunks a one-process `score` cuts the chromosome into so that a chunk's genotypes
    fit the GPU: 1 (the reference's one-process form, sai.py:86-93 with one worker) unless the file promises more
    int8 genotype bytes than the budget -- then ceil(bytes / budget), the grain the sharded route already uses
    (chunk_generator.py:111-142), chunk after chunk through the same GPU, the output files byte-identical.
    The estimate is the file's: a genotype is about four bytes of VCF text ("0|1" + tab; bgzip shrinks genotype
    text about twelvefold), of which one int8 dosage stays resident -- besides the reader's staging and the tiled
    copy per population, hence a budget of a quarter of the free HBM.  ``SAI_AMD_HBM_BUDGET_BYTES`` overrides it.
    A PLINK ``.bed`` and a packed ``.geno`` hold four genotypes per byte: 4 x their size stays resident; a text
    ``.geno`` holds one: 1 x.  With ``layout="packed2"`` a ``.bed`` is never widened: 1 x its size stays resident; a
    ``.pgen`` is compressed, so its header's counts say it: variant_ct x ceil(sample_ct / 4).  ``src_file`` (int8 layout): the
    source file's own estimate is added to the main input's -- both blocks are resident while they are joined; with several
    source files (a list or tuple), every file's."""
    from .site_join_many import as_list
    from .utils.filesets import resident_bytes

    try:
        resident = resident_bytes(vcf_file)
        if layout == "packed2" and resident is not None:
            from .utils import pgen, plink
            from .utils.filesets import reader_for

            if reader_for(vcf_file) is pgen:
                variant_ct, sample_ct = pgen.header_counts(vcf_file)
                resident = variant_ct * -(-sample_ct // 4)
            else:
                resident = os.path.getsize(plink.fileset_prefix(vcf_file) + ".bed")
        if resident is None:
            size = os.path.getsize(vcf_file)
            resident = size * 3 if str(vcf_file).endswith((".gz", ".bgz")) else size // 4
        for f in as_list(src_file):
            second = resident_bytes(f)
            if second is None:
                size = os.path.getsize(f)
                second = size * 3 if str(f).endswith((".gz", ".bgz")) else size // 4
            resident += second
    except OSError:
        return 1
    raw = os.environ.get("SAI_AMD_HBM_BUDGET_BYTES", "")
    if raw:
        budget = int(raw)
        if budget < 1:
            raise ValueError("SAI_AMD_HBM_BUDGET_BYTES must be a positive integer")
    else:
        try:
            import torch

            if not torch.cuda.is_available():
                return 1
            budget = torch.cuda.mem_get_info()[0] // 4
        except (ImportError, RuntimeError):
            return 1
    return max(1, -(-resident // max(budget, 1)))


def _score_over_ranks(vcf_file, chr_name, win_len, win_step, anc_allele_file, output_file, config, src_file=None) -> None:
    """This process is one rank of a launched job: take the sharded route and leave the group cleanly."""
    from .distributed import score_sharded, shutdown_process_group
    from .launcher import chunks_per_worker

    second = {} if src_file is None else {"src_file": src_file}
    try:
        score_sharded(vcf_file, chr_name, win_len, win_step, anc_allele_file, output_file, config,
                      chunks_per_rank=chunks_per_worker(), **second)  # fmt: skip
    finally:
        shutdown_process_group()


def _score_cli_arguments(vcf_file, chr_name, win_len, win_step, anc_allele_file, output_file, config, num_workers, src_file=None) -> list:
    from .site_join_many import as_list
    from .utils.filesets import cli_source

    argv = ["score", *cli_source(vcf_file), "--chr-name", chr_name, "--win-len", win_len, "--win-step", win_step,
            "--output", output_file, "--config", config, "--num-workers", num_workers]  # fmt: skip
    if anc_allele_file is not None:
        argv += ["--anc-alleles", anc_allele_file]
    for f in as_list(src_file):
        argv += ["--src-input", f]  # once per source file
    return [str(a) for a in argv]


def score(vcf_file: str, chr_name: str, win_len: int, win_step: int, anc_allele_file: str, output_file: str, config: str,
          num_workers: int, layout: str = None, *, src_file: str = None) -> None:  # fmt: skip
    """Sliding-window scores of one chromosome, written as the reference writes them (TSV +
    ``.U.log`` + ``.Q.log``; interface of sai.py:33-42).

    ``num_workers`` is the reference's worker-process count (sai.py:42, grain ``num_workers * 8`` chunks at
    :91) with one process per GPU: 1 computes every window in this process; N > 1 starts N ranks as a
    child job (``sai_amd.launcher``: before this process has touched the GPU) whose ranks cut the window
    list into ``N * 8`` ChunkGenerator chunks, each rank reading and scoring its own contiguous share on
    its own GPU, with one final gather to rank 0, which writes the files -- byte-identical to the
    one-process files for any N (``sai_amd.distributed.score_sharded``).  Inside such a job
    (``WORLD_SIZE`` > 1: torchrun's environment) the call IS a rank and takes the sharded route.

    ``layout`` = ``"int8"`` (the default; ``SAI_AMD_LAYOUT`` overrides it) or ``"packed2"``: a PLINK 1 or PLINK 2 fileset
    is decoded straight into the 2-bit layout and U, Q, fd, df, Danc and Dplus are scored on it -- four times as many sites
    per chunk, the same files byte for byte.  What that route cannot serve (DD among the statistics) is a ValueError
    before anything is read (``require_packed2_input``); a missing call in a row flipped by the ancestral allele (dosage 4
    at ploidy 2) is one while reading: with ``anc_allele_file`` -- which fd, df, Danc and Dplus require -- the layout serves
    panels without a missing call in a flipped row, and the message names the int8 layout for the others.

    ``src_file``: the samples of the configuration's ``src`` list are read from this file -- anything ``vcf_file`` may be:
    a plain, gzip or bgzip VCF, a BCF, ``PREFIX.bed`` / ``.geno`` / ``.pgen`` -- and those of the other lists from
    ``vcf_file``; both are polarised by ``anc_allele_file``, which is required, and scored over the sites both readers kept
    (``sai_amd.site_join``), in the int8 layout.  THE WINDOW GRID IS THE MAIN INPUT'S: ``ChunkGenerator`` and the one-pass
    scan read ``vcf_file`` as before; the source file contributes genotypes, not windows.  What cannot be served is
    refused before the output directory is made (``require_second_input``).  A list or tuple of 2 to 16 paths (a sequence of
    one is that path): one file per archaic individual or per lab; every sample of the ``src`` list must be held by exactly
    one of the files and every file must hold one, the sites are those ALL inputs hold, and the individuals of a population
    stand in the order of the ``src`` list (``sai_amd.site_join_many``)."""
    from . import launcher

    num_workers = 1 if num_workers is None else int(num_workers)
    if num_workers < 1:
        raise ValueError("`num_workers` must be a positive integer.")
    layout = resolve_layout(layout)
    second = {}
    if src_file is not None:
        from .site_join_many import is_many, require_sources, source_files

        src_file = source_files(src_file)  # the str of one file, or the list of several
        require_second_input(vcf_file, src_file, anc_allele_file, layout)
        if is_many(src_file):  # which sample comes from which file: every src sample from exactly one, every file holding one
            cfg = load_config(config)
            require_sources(src_file, cfg.ploidies, cfg.populations.get_population("src"))
        second = {"src_file": src_file}
    if layout == "packed2":
        require_packed2_input(vcf_file, config, num_workers)
    if launcher.in_rank_job():
        _score_over_ranks(vcf_file, chr_name, win_len, win_step, anc_allele_file, output_file, config, **second)
        return
    if num_workers > 1:
        # the errors a one-process run raises before any work (configuration, polarisation) are raised here,
        # by the caller's own process, not as a failed child job
        cfg = load_config(config)
        require_polarised_input(cfg.statistics, anc_allele_file)
        rc = launcher.launch_ranks(
            num_workers, _score_cli_arguments(vcf_file, chr_name, win_len, win_step, anc_allele_file, output_file, config, num_workers, **second),
            module="sai_amd", who="sai score")  # fmt: skip
        if rc != 0:
            raise launcher.RankJobFailed(num_workers, rc)
        return
    cfg = load_config(config)
    require_polarised_input(cfg.statistics, anc_allele_file)
    driver = chunk_preprocessor_for(cfg, vcf_file, win_len, win_step, output_file, anc_allele_file, layout=layout, **second)
    span, preloaded = None, None
    n_chunks = chunks_for_memory(vcf_file, layout, **second)  # 1 unless the chromosome's genotypes would not fit the GPU at once
    if n_chunks == 1 and _reads_in_one_pass(vcf_file):
        span, preloaded = _scan_while_reading(driver, vcf_file, str(chr_name))
    chunks = ChunkGenerator(vcf_file=vcf_file, chr_name=chr_name, window_size=win_len, step_size=win_step,
                            num_chunks=n_chunks, span=span)  # fmt: skip
    write_headers(output_file, cfg.statistics, cfg.ploidies)
    # numeric batches -> text, natively; the item-dictionary route (driver.run + process_items)
    # writes the same bytes and stays what plug-ins and the sharded executors use
    tasks = list(chunks.get())
    if len(tasks) == 1:  # the usual run: the rows of the first windows are written while the GPU scores the later ones
        chunk = tasks[0]
        fits = preloaded is not None and (preloaded[2] is None or (chunk["start"] <= preloaded[2][0] and preloaded[2][1] <= chunk["end"]))
        driver.run_and_write(**chunk, preloaded=preloaded[:2] if fits else None)
    else:  # chunk after chunk through the GPU; the files are combination-major, so the rows wait for the last chunk
        driver.write_results([driver.run_compact(**chunk) for chunk in tasks])
    if os.environ.get("SAI_AMD_KEEP_INGEST_BUFFERS", "1") == "0":
        # the readers' staging (about 650 MB of HBM + 125 MB pinned for a large bgzip file) is kept for the
        # next call by default -- allocating and page-locking it costs more than a small `score`
        from .engine import Engine
        from .utils.filesets import release_buffers

        Engine.get().release_ingest_buffers()
        release_buffers(Engine.get())


def convert(vcf_file: str, chr_name: str, out_prefix: str = None, ploidy: int = 2, haploid_samples=None, samples=None, start: int = None,
            end: int = None, append: bool = False, skip_multiallelic: bool = False, out_pfile: str = None, out_eigenstrat: str = None,
            geno_format: str = "packed", labels=None, ld_compress: bool = False) -> dict:  # fmt: skip
    """Write one chromosome of a VCF (plain, gzip or bgzip) as the PLINK 1 fileset ``out_prefix`` (.bed / .bim / .fam),
    as the PLINK 2 fileset ``out_pfile`` (.pgen / .pvar / .psam: about a third of the .bed's bytes) or as the EIGENSOFT
    fileset ``out_eigenstrat`` (.geno / .snp / .ind, what ADMIXTOOLS reads; ``geno_format`` = "packed", the default, or
    "transposed"; ``labels`` = sample name -> population label of its ``.ind`` line), encoded on the
    GPU: not a command of the reference.  Reading the fileset at the ploidies it was written with gives the block the
    VCF reader gives, byte for byte, so ``score`` on it writes the same files -- from either layout.  The arguments,
    the summary it returns and the refusals: ``utils.bed_writer.convert``, ``utils.pgen_writer.convert`` and
    ``utils.geno_writer.convert``.  ``ld_compress``, with ``out_pfile`` only, also writes rows as their differences
    from an earlier row (record types 2 and 3): a smaller file of a panel whose neighbouring variants resemble each other,
    the same block when it is read.  The
    ``.pgen`` rules were written from memory of the specification: the output is read back by this project's readers
    and equals its test writer's, and has not been opened with plink2.  The two hashes in the header record of a
    ``.geno`` were written from memory of EIGENSOFT's ``hasharr`` and are unverified; ``hashcheck: NO`` in a
    ``convertf`` / ADMIXTOOLS parameter file is the way around a mismatch."""
    given = [name for name, value in (("out_prefix", out_prefix), ("out_pfile", out_pfile), ("out_eigenstrat", out_eigenstrat)) if value is not None]
    if len(given) != 1:
        raise ValueError("convert writes one fileset: name either out_prefix (PLINK 1) or out_pfile (PLINK 2) or out_eigenstrat (EIGENSOFT)"
                         + (f", not {' and '.join(given)}" if given else ""))  # fmt: skip
    if out_eigenstrat is None and (geno_format != "packed" or labels is not None):
        raise ValueError("geno_format and labels go with out_eigenstrat: the PLINK filesets have one form and no population column")
    if ld_compress and out_pfile is None:
        raise ValueError("ld_compress goes with out_pfile: only a .pgen holds records that list their differences from an earlier record")
    common = dict(ploidy=ploidy, haploid_samples=haploid_samples, samples=samples, start=start, end=end, append=append, skip_multiallelic=skip_multiallelic)
    if out_eigenstrat is not None:
        from .utils.geno_writer import convert as write_geno

        return write_geno(vcf_file, chr_name, out_eigenstrat, geno_format=geno_format, labels=labels, **common)
    if out_pfile is not None:
        from .utils.pgen_writer import convert as write_fileset

        if ld_compress:
            common["ld_compress"] = True
    else:
        from .utils.bed_writer import convert as write_fileset

    return write_fileset(vcf_file, chr_name, out_prefix if out_pfile is None else out_pfile, **common)


def outlier(score_file: str, output_prefix: str, quantile: float) -> None:
    """Per statistic column of a score table, write the rows beyond the ``quantile`` of that
    column to ``{output_prefix}.{column}.{quantile}.outliers.tsv`` (sai.py:154-230): columns
    after ``N(Variants)`` are statistics; ``U*`` columns keep rows strictly above the threshold,
    the others rows at or above it; a column without numbers, or with a single distinct value,
    gives a header-only file and a UserWarning; rows are naturally sorted by Chrom/Start/End.
    Host-side post-processing of a small table (pandas, like the reference); no GPU involved."""
    import pandas as pd

    from .utils import natsorted_df

    df = pd.read_csv(score_file, sep="\t", na_values=["nan"], index_col=False)
    cols = list(df.columns)
    if "N(Variants)" in cols:
        metric_cols = cols[cols.index("N(Variants)") + 1 :]
    else:  # sai.py:188-194
        skip = {"Chrom", "Start", "End", "Ref", "Tgt", "Src"}
        metric_cols = [c for c in cols if c not in skip and pd.to_numeric(df[c], errors="coerce").notna().any()]
    if not metric_cols:
        raise ValueError("No metric columns found.")
    for col in metric_cols:
        numeric = pd.to_numeric(df[col], errors="coerce")
        present = numeric.dropna()
        if present.empty:
            warnings.warn(f"Column '{col}' has no numeric values; writing empty result.", UserWarning)
            out = pd.DataFrame(columns=df.columns)
        elif present.nunique() == 1:
            warnings.warn(
                f"Column '{col}' has only one unique value ({present.iloc[0]}); writing empty result.", UserWarning
            )
            out = pd.DataFrame(columns=df.columns)
        else:
            thr = present.quantile(quantile)
            out = df[numeric > thr] if col.startswith("U") else df[numeric >= thr]
            if not out.empty:
                out = natsorted_df(out.reset_index(drop=True))
        out.astype(str).to_csv(f"{output_prefix}.{col}.{quantile}.outliers.tsv", index=False, sep="\t")
