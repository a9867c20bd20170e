"""What the probing site pass is expected to read on C3's block, counted from the data (a read-all pass's counts and the
probe rows themselves): tiles that exit at the source vote, after the probe, before the target, and tiles read whole.
python tools/ref_probe_census.py [n_sites]   -> the tile counts and the expected bytes per launch"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from sai_amd.engine import Engine
from sai_amd.resident import synth_block

n_sites = int(float(sys.argv[1])) if len(sys.argv) > 1 else int(1e7)
n_ref = n_tgt = 1000
w, ploidy = 0.01, 2
eng = Engine.get(0)
P = int(eng.lib.sai_ref_probe_rows())
block = synth_block(eng, bench.SEED0 + 3, 1, n_sites, n_ref, n_tgt, [2])
counts = eng.site_counts(block.pops).to(torch.int64)  # [pops][sites][2]
n_tiles = -(-n_sites // 64)
f = [counts[p, :, 0].double() / (counts[p, :, 1] * ploidy).double() for p in range(3)]  # 0 / 0 = NaN: no comparison holds
hit = (f[2] == 1.0)
rows = block.pops[0].tiles.reshape(-1)[: n_tiles * n_ref * 64].view(n_tiles, n_ref, 64)
partial = torch.cat([rows[t : t + 8192, :P].clamp(min=0).sum(dim=1, dtype=torch.int32) for t in range(0, n_tiles, 8192)]).reshape(-1)[:n_sites]
may_probe = hit & (partial.double() / float(n_ref * ploidy) < w)
may_whole = hit & (f[0] < w) & (f[0] >= 0)
per_tile = lambda b: torch.nn.functional.pad(b, (0, n_tiles * 64 - n_sites)).view(n_tiles, 64).any(dim=1)  # noqa: E731
t_hit, t_probe, t_whole = (int(per_tile(b).sum()) for b in (hit, may_probe, may_whole))
src = 64 * 2
expected = n_tiles * src + t_hit * 64 * P + t_probe * 64 * (n_ref - P) + t_whole * 64 * n_tgt
print(f"{n_tiles} tiles: {n_tiles - t_hit} exit at the source vote, {t_hit - t_probe} after the {P}-row probe, {t_probe - t_whole} before the target, "
      f"{t_whole} are read whole ({int(may_whole.sum())} sites pass)")
print(f"expected bytes per launch: {n_tiles} x {src} + {t_hit} x {64 * P} + {t_probe} x {64 * (n_ref - P)} + {t_whole} x {64 * n_tgt} = {expected}")
