"""``ResidentScorer(layout="packed2")`` over populations that are packed already.

``ResidentScorer`` re-encodes the tiled int8 populations of its block with ``Engine.pack2`` when it is built.  A
PLINK 1 or PLINK 2 fileset read with ``layout="packed2"`` arrives as ``PackedPop`` blocks (``plink.load_packed_device``
/ ``pgen.load_packed_device``: the ``.bed`` rows or ``.pgen`` records decoded straight into the layout), and those are streamed as they are: the scorer is handed the engine
through ``_KeepPacked``, whose ``pack2`` passes a ``PackedPop`` through and re-encodes anything else.  Everything
else of the scorer -- the fused packed2 site pass, the windows stage, the records -- is ``ResidentScorer``'s own.

(It lives beside ``resident.py`` and not in it: the stored figures under profiles/ name the digest of the sources
they were measured on -- ``bench.source_digest``: ``resident.py`` and ``engine.py`` among them -- and this route
changes nothing those figures depend on.)
"""

from __future__ import annotations

from .engine import PackedPop
from .resident import ResidentBlock, ResidentScorer


class _KeepPacked:
    """The engine as ``ResidentScorer`` sees it; ``pack2`` of a population that is packed already is that population."""

    def __init__(self, eng):
        self._eng = eng

    def pack2(self, pop):
        return pop if isinstance(pop, PackedPop) else self._eng.pack2(pop)

    def __getattr__(self, name):
        return getattr(self._eng, name)


def packed_scorer(eng, block: ResidentBlock, windows, sets, **kw) -> ResidentScorer:
    """``ResidentScorer(eng, block, windows, sets, layout="packed2", **kw)`` for a block whose populations may be
    ``PackedPop``: no ``Engine.pack2`` pass over those, no int8 block behind them."""
    if any(isinstance(p, PackedPop) and p.n_sites != block.pops[0].n_sites for p in block.pops):
        raise ValueError("all populations of a block must cover the same sites")
    return ResidentScorer(_KeepPacked(eng), block, windows, sets, layout="packed2", **kw)
