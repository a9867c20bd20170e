"""What the two readers that decode a fileset straight into the packed2 layout share (``plink.load_packed*``,
``pgen.load_packed*``): the populations of a read as slices of one index, and how a flagged row becomes the reader's
ValueError."""

from __future__ import annotations

import numpy as np


def _packed_bytes(n_sites: int, n_ind: int) -> int:
    """``sai_packed2_bytes`` (saihip.h), restated for the host readers: the sanitizer build has no kernel unit."""
    return -(-n_sites // 64) * ((n_ind // 64) * 256 + ((n_ind % 64 + 15) // 16) * 64) * 4


class _PackedPlan:
    """The populations of a packed read as slices of ONE index: population p holds the slots [lo, hi) of it, at one
    ploidy, and ``first_col`` >= 0 when its samples are a run of consecutive sample columns (the kernel's fast path).
    ``make_index(samples, ploidies)`` builds the format's index; ``whole_row`` = its status codes that stand for a
    row, not a slot; ``ext`` and ``variant_id`` = the data file's extension and the module's ``_variant_id``."""

    def __init__(self, make_index, populations, whole_row, ext: str, variant_id):
        samples = [name for names, _ in populations for name in names]
        ploidies = [int(ploidy) for names, ploidy in populations for _ in names]
        self.idx = make_index(samples, ploidies)
        self.whole_row, self.ext, self.variant_id = whole_row, ext, variant_id
        self.pops, lo = [], 0
        for names, ploidy in populations:
            cols = np.ascontiguousarray(self.idx.col_of_slot[lo : lo + len(names)])
            run = len(cols) > 0 and np.array_equal(cols, np.arange(cols[0], cols[0] + len(cols), dtype=np.int32))
            self.pops.append({"lo": lo, "n_ind": len(names), "ploidy": int(ploidy), "cols": cols, "first_col": int(cols[0]) if run else -1})
            lo += len(names)

    def raise_flagged(self, status, unfit) -> None:
        """``status`` / ``unfit`` = per population the int32 array over the rows of the index, or None when nothing is
        flagged there.  A refused row (whatever the int8 route refuses: a heterozygous call at ploidy 1, an index out
        of range, a record that does not parse) is reported first, in the words of the int8 route: the first such row,
        and in it the lowest slot of the request.  Then the first row that does not fit two bits."""
        idx = self.idx
        for flags, report in ((status, self._refused), (unfit, self._unfit)):
            rows = [int(np.flatnonzero(f)[0]) if f is not None and f.any() else idx.n_rows for f in flags]
            k = min(rows, default=idx.n_rows)
            if k < idx.n_rows:
                p = rows.index(k)  # populations in request order: the first one flagged holds the lowest slot
                report(k, self.pops[p], int(flags[p][k]))

    def raise_flagged_device(self, flags) -> None:
        """``raise_flagged`` for the device readers' ``flags``: int32 [population][status, unfit][row] in HBM."""
        live = [p for p, pop in enumerate(self.pops) if pop["n_ind"]]
        if any(bool(flags[p].any()) for p in live):  # per population: a view, no copy of the flags
            host = flags.cpu().numpy()
            self.raise_flagged([host[p, 0] if p in live else None for p in range(len(self.pops))],
                               [host[p, 1] if p in live else None for p in range(len(self.pops))])  # fmt: skip

    def _refused(self, k: int, pop: dict, st: int) -> None:
        one = np.zeros(1, dtype=np.int32)
        one[0] = st if st in self.whole_row else self.idx.n_slots - (pop["lo"] + pop["n_ind"] - st)
        self.idx.raise_flagged(one, k)

    def _unfit(self, k: int, pop: dict, uf: int) -> None:
        idx = self.idx
        sample = idx.samples[pop["lo"] + pop["n_ind"] - uf]
        raise ValueError(
            f"{idx.prefix}{self.ext}: missing call of sample {sample} at variant {self.variant_id(idx.prefix, int(idx.file_row[k]))} "
            f"(position {int(idx.pos[k])}) in a row flipped by the ancestral allele: its dosage is 4, which the 2-bit layout "
            "cannot hold; read this fileset with --layout int8"
        )

    def device_blocks(self, eng) -> list:
        """One empty ``PackedPop`` per population in HBM: what a device read fills."""
        import torch

        from ..engine import PackedPop

        packed = []
        for pop in self.pops:
            nbytes = int(eng.lib.sai_packed2_bytes(self.idx.n_rows, pop["n_ind"]))
            if nbytes < 0:
                raise ValueError("packed2: population too large")
            packed.append(PackedPop(torch.empty((nbytes,), dtype=torch.uint8, device=eng.device), self.idx.n_rows, pop["n_ind"]))
        return packed
