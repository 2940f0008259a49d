"""The one owner of the GroupNorm statistics that producers leave for consumers: per-slot column sums [slots][2][n] (fp32, zeroed) of
an output tensor, written by the producing kernel's epilogue and read by the GroupNorm that follows.  Producers ask `produce`, consumers
ask `consume`, `follow` carries them over a batch duplication.  Every decision depends on shapes only and memory comes from the injected
allocator, so the rules (tests/test_gn_stats_host.py) hold without a device.
"""
from __future__ import annotations

import torch

# statistics ride on the producer's epilogue from this many output rows on (below, the GEMMs are split-K launches whose reduce pass owns
# the epilogue, and a one-launch GroupNorm is as cheap as the finalize + apply pair)
GN_STATS_MIN_M = 16384


class GnStats:
    def __init__(self, alloc):
        self.alloc = alloc              # alloc(*shape, dtype=, zero=) -> tensor (LaunchRecorder.buf)
        self.fuse_gn_stats = True
        self._cs = {}                   # (data_ptr of a producer's output, rows per slot) -> its column-sum buffer

    def _new(self, t, slots, n, rows_per_slot):
        cs = self._cs[t.data_ptr(), rows_per_slot] = self.alloc(slots, 2, n, dtype=torch.float32, zero=True)
        return cs

    def produce(self, out, kind, *, rows, n, hw=0, asked=True, z=1, w=0):
        """The producer of `out` ([rows, n], hw rows per sample) was asked to leave statistics: the buffer its epilogue fills, or None.
        kind: "gemm" (z launches batched over z), "phase" (the four sub-pixel launches of an upsampling convolution share the buffer: phase p
        of sample b owns a quarter of b's slots, so a quarter of hw must be whole slots), "winograd" (output transform of feature maps
        w wide: one image row = one slot), "xtail" -- all 32-row slots -- and "tile" (halo-patch convolutions: one slot per 16 x 16 tile)."""
        if not (asked and self.fuse_gn_stats):
            return None
        if kind == "tile":
            return self._new(out, rows // 256, n, 256)
        ok = {"gemm": z == 1 and rows % 32 == 0, "phase": (hw // 4) % 32 == 0, "winograd": w == 32 and n % 128 == 0, "xtail": True}[kind]
        return self._new(out, rows // 32, n, 32) if ok and rows >= GN_STATS_MIN_M else None

    def consume(self, x0, x1=None, *, hw, accepts=(32,)):
        """Statistics for a GroupNorm over x0 (| x1) with hw rows per sample -> (colstats0, colstats1, rows per slot), colstats0 None when
        a source has none the consumer can use.  accepts: the slot sizes the consumer reads, in order of preference; 32-row slots must not
        straddle samples."""
        xs = [x for x in (x0, x1) if x is not None]
        for rps in accepts:
            cs = [self._cs.get((x.data_ptr(), rps)) for x in xs]
            if all(c is not None for c in cs) and (rps != 32 or hw % 32 == 0):
                return cs[0], (cs[1] if x1 is not None else None), rps
        return None, None, 32

    def follow(self, src, dst):
        """dst = [src | src] along the batch axis: src's 32-row statistics get a buffer of twice the slots -> (theirs, dst's) for the
        caller to copy, or None.  (Per-tile statistics do not follow: no duplicated tensor feeds a table consumer.)"""
        cs = self._cs.get((src.data_ptr(), 32))
        return None if cs is None else (cs, self._new(dst, 2 * cs.shape[0], cs.shape[2], 32))
