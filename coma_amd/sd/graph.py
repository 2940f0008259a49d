"""The diffusion operator vocabulary over the launch recorder (sd/recorder.py): a network is compiled ONCE into a flat list of kernel
launches over pre-allocated NHWC fp16 buffers.  This replaces the per-op Python dispatch of the reference's diffusers modules -- the
MI355X-first equivalent of a tracing compiler is "hipGraph over hand-written kernels", not op-by-op eager execution.  Which producer
leaves GroupNorm statistics and which consumer may read them is decided in one place, sd/gn_stats.py.
"""
from __future__ import annotations

import torch

from . import ops
from .gn_stats import GnStats
from .recorder import F16, LaunchRecorder  # noqa: F401  (F16 is re-exported: the network builders import it from here)


class LaunchGraph(LaunchRecorder):
    def __init__(self, device, model=None, plan="step"):
        super().__init__(device, model, plan)
        self._gn_scratch = None
        self._ws = None             # split-K workspace shared by every GEMM of the graph (launches are serial)
        self.gn_stats = GnStats(self.buf)

    def gn_scratch(self, batch, hw):
        n = ops.gn_scratch_floats(batch, hw)
        if self._gn_scratch is None or self._gn_scratch.numel() < n:
            self._gn_scratch = self.buf(max(n, 1 << 16), dtype=torch.float32)
        return self._gn_scratch

    def conv(self, a0, w, out, *, batch, in_h, in_w, c0, n, out_h=None, out_w=None, a1=None, c1=0, taps=1, **kw):
        oh = out_h if out_h is not None else in_h
        ow = out_w if out_w is not None else in_w
        z = kw.get("nbatch_z", 1)
        if self._ws is None:
            self._ws = self.buf(16 << 20, dtype=torch.float32)   # 64 MiB
        kw.setdefault("workspace", self._ws)
        M = batch * oh * ow
        alg_flops = kw.pop("alg_flops", None)
        tag_note = kw.pop("tag_note", "")
        # GroupNorm statistics of the consumer come for free from the epilogue of large, never-split GEMMs
        cs = self.gn_stats.produce(out, "gemm", rows=M, n=n, hw=oh * ow, asked=kw.pop("stats", False), z=z)
        if cs is not None:
            kw["colstats"] = cs
        self.add(lambda: ops.conv_gemm(a0, w, out, batch=batch, in_h=in_h, in_w=in_w, out_h=oh, out_w=ow, c0=c0, n=n, a1=a1,
                                       c1=c1, taps=taps, **kw),
                 flops=2 * batch * oh * ow * n * taps * (c0 + c1) * z, alg_flops=alg_flops,
                 # unique bytes: the input activation(s), the weights (shared over z unless strided), bias / residual, the output
                 nbytes=2 * (z * batch * in_h * in_w * (c0 + c1) + (z if kw.get("stride_w") else 1) * n * taps * (c0 + c1)
                             + z * M * (n // 2 if kw.get("epi", 0) & ops.EPI_GEGLU else n) * (2 if kw.get("res") is not None else 1)
                             + (n if kw.get("bias") is not None else 0) + (batch * n if kw.get("bias_bn") is not None else 0)),
                 tag=f"gemm M={batch * oh * ow} N={n} K={taps * (c0 + c1)} taps={taps} z={z}" + tag_note)
        return out

    def conv3x3_upsampled(self, a0, w_raw, out, *, batch, in_h, in_w, c0, n, bias=None, stats=False, one_launch=False):
        """diffusers Upsample2D: conv3x3(nearest-upsample-x2(a0)) as FOUR sub-pixel phase products over the source (sd_conv_gemm_desc.phase):
        16 multiplies per output 2 x 2 block instead of 36, exact (the folded weights are sums of the 3x3 taps), no transformed tensors.
        w_raw: the torch-layout weight [n, c0, 3, 3]; out: [batch * 2 in_h * 2 in_w, n].
        one_launch: the four products as the z dimension of ONE launch (phase = 5) -- their tiles fill the chip together where a single
        phase is a round of one tile per CU (the 640-channel upsampler of the UNet)."""
        from .weights import upsample_phase_weights
        assert in_w & (in_w - 1) == 0, "phase launches need a power-of-two source width"
        M = batch * in_h * in_w
        ws = upsample_phase_weights(w_raw)
        cs = self.gn_stats.produce(out, "phase", rows=4 * M, n=n, hw=4 * in_h * in_w, asked=stats)      # ONE buffer for the four phases
        if one_launch:
            self.conv(a0, torch.stack(ws).contiguous(), out, batch=batch, in_h=in_h, in_w=in_w, c0=c0, n=n, taps=4, phase=5, nbatch_z=4,
                      stride_w=n * 4 * c0, bias=bias, colstats=cs, alg_flops=2 * 4 * M * n * 9 * c0, tag_note=" (upsample, four phases)")
            return out
        for ph in range(4):
            self.conv(a0, ws[ph], out, batch=batch, in_h=in_h, in_w=in_w, c0=c0, n=n, taps=4, phase=ph + 1, bias=bias, colstats=cs,
                      alg_flops=2 * M * n * 9 * c0, tag_note=f" (upsample phase {ph})")
        return out

    # ---- Winograd F(2x2,3x3) for the deep ResNet levels (profiles/r04_notes.md 1, 4): input transform -> 16 plane products (the 1x1 GEMM
    # path, nbatch_z = 16) -> output transform with the epilogue.  2.25 x fewer MFMA flops; only worth it where the 4 x larger transformed
    # tensors stay in the Infinity Cache and K = C_in is long -- the 16 x 16 / 8 x 8 levels of the UNet.
    # fp16 headroom of the STORED planes (sd_hip.h "fp16 range"): U carries 1/4, and V another 1/4 where the input is an un-normalised
    # tensor (the Upsample2D convolutions: V alone reaches 4 max|d|); the output transforms multiply by 4 / 16 in fp32 -- exact.
    WINO_USCALE = 0.25
    WINO_VSCALE_RAW = 0.25

    def winograd_weight(self, w9, *, n, c):
        """w9 fp16 [n][9 * c] (the direct kernel's layout) -> U fp16 [16][n][c] = WINO_USCALE * G g G^T, computed once, here."""
        U = torch.empty(16, n, c, dtype=torch.float16, device=self.device)        # constants: registered PERSISTENT when first recorded
        ops.winograd_weight(w9, U, n=n, c=c, uscale=self.WINO_USCALE)
        return U

    def winograd_planes(self, V, U, *, tiles, c, n):
        P = self.buf(16, tiles, n)
        self.conv(V, U, P, batch=tiles, in_h=1, in_w=1, c0=c, n=n, nbatch_z=16, stride_a=tiles * c, stride_w=n * c, stride_out=tiles * n,
                  alg_flops=2 * 9 * (4 * tiles) * n * c, tag_note=" (winograd planes)")      # counted as the 3x3 convolution these 16 products compute
        return P

    def winograd_input(self, a0, *, batch, h, w, c0, a1=None, c1=0, upsample=False, vscale=1.0):
        C, T = c0 + c1, batch * (h // 2) * (w // 2)
        V = self.buf(16, T, C)
        self.add(lambda: ops.winograd_input(a0, V, batch=batch, h=h, w=w, c0=c0, x1=a1, c1=c1, upsample=upsample, vscale=vscale),
                 tag=f"winograd input{' (upsampled)' if upsample else ''} B={batch} {h}x{w} C={C}", nbytes=2 * 5 * batch * h * w * C)
        return V

    GN_WINO_MAX_SLICE = 20480

    def gn_winograd_input(self, gamma, beta, *, batch, h, w, c0, x0=None, x1=None, c1=0, m=None, bias=None, bias_bn=None, ldbb=0, eps, silu=True,
                          groups=32, vscale_of_m=1.0):
        """GroupNorm (+ SiLU) -> Winograd input transform in ONE launch (sd_gn_winograd_input_f16); the source is [x0 | x1] or the plane
        products `m` of the previous Winograd convolution (its output transform, bias and per-sample bias happen here)."""
        C, T = c0 + c1, batch * (h // 2) * (w // 2)
        assert h * w * (C // groups) <= self.GN_WINO_MAX_SLICE
        V = self.buf(16, T, C)
        self.add(lambda: ops.gn_winograd_input(V, gamma, beta, batch=batch, h=h, w=w, c0=c0, x0=x0, x1=x1, c1=c1, m=m, ldm=c0, bias=bias,
                                               bias_bn=bias_bn, ldbb=ldbb, groups=groups, eps=eps, silu=silu, mscale=1.0 / (self.WINO_USCALE * vscale_of_m)),
                 tag=f"groupnorm + winograd input{' (from planes)' if m is not None else ''} B={batch} {h}x{w} C={C}",
                 nbytes=2 * (5 + (16 if m is not None else 1)) * batch * h * w * C // (4 if m is not None else 1))
        return V

    def winograd_output(self, P, out, *, batch, h, w, n, bias=None, bias_bn=None, ldbb=0, res=None, stats=False, vscale=1.0):
        """stats: also leave the column sums of `out` for the consumer's GroupNorm (w = 32 only: one image row = one 32-row slot).
        vscale: the scale the producer of V applied (the planes are WINO_USCALE * vscale times the true products)."""
        mscale = 1.0 / (self.WINO_USCALE * vscale)
        cs = self.gn_stats.produce(out, "winograd", rows=batch * h * w, n=n, hw=h * w, asked=stats, w=w)
        self.add(lambda: ops.winograd_output(P, out, batch=batch, h=h, w=w, n=n, bias=bias, bias_bn=bias_bn, ldbb=ldbb, res=res, colstats=cs, mscale=mscale),
                 tag=f"winograd output{' (+ colstats)' if cs is not None else ''} B={batch} {h}x{w} N={n}",
                 nbytes=2 * (5 + (1 if res is not None else 0)) * batch * h * w * n)
        return out

    def gn_table_winograd_input(self, x0, gamma, beta, *, batch, h, w, c0, x1=None, c1=0, eps, silu=True):
        """GroupNorm (+ SiLU) folded into the input transform through the per-(sample, channel) affine table, for slices too large for
        gn_winograd_input: needs the column sums of every source (left by its producer); returns None when one is missing.  Two launches
        (table, transform), and the normalised tensor is never written."""
        table = self._table(x0, gamma, beta, batch=batch, hw=h * w, c=c0, eps=eps, x1=x1, c1=c1, accepts=(32,), from_stats_only=True)
        if table is None:
            return None
        C, T = c0 + c1, batch * (h // 2) * (w // 2)
        V = self.buf(16, T, C)
        self.add(lambda: ops.winograd_input(x0, V, batch=batch, h=h, w=w, c0=c0, x1=x1, c1=c1, gn_affine=table, silu=silu),
                 tag=f"groupnorm apply + winograd input B={batch} {h}x{w} C={C}", nbytes=2 * 5 * batch * h * w * C)
        return V

    def conv3x3_winograd(self, a0, w9, out, *, batch, in_h, in_w, c0, n, a1=None, c1=0, bias=None, bias_bn=None, ldbb=0, res=None, upsample=False,
                         stats=False):
        """The unfused chain: input transform -> plane products -> output transform (+ bias, per-sample bias, residual).  in_h, in_w are
        the convolution's own (= output) resolution; with upsample the sources are [in_h / 2, in_w / 2]."""
        C, T = c0 + c1, batch * (in_h // 2) * (in_w // 2)
        vs = self.WINO_VSCALE_RAW       # the caller's tensor is not known to be normalised (the UNet's Upsample2D convolutions use this chain)
        V = self.winograd_input(a0, batch=batch, h=in_h, w=in_w, c0=c0, a1=a1, c1=c1, upsample=upsample, vscale=vs)
        P = self.winograd_planes(V, self.winograd_weight(w9, n=n, c=C), tiles=T, c=C, n=n)
        return self.winograd_output(P, out, batch=batch, h=in_h, w=in_w, n=n, bias=bias, bias_bn=bias_bn, ldbb=ldbb, res=res, stats=stats, vscale=vs)

    def dup(self, src, dst):
        """dst = [src | src] along the batch axis (two identical CFG halves); the GroupNorm column sums of src follow."""
        assert dst.numel() == 2 * src.numel()
        self._dup(src, dst, tag=f"dup {src.numel() * 2 >> 20} MiB")
        cs = self.gn_stats.follow(src, dst)
        if cs is not None:
            self._dup(*cs, tag="dup colstats")
        return dst

    def _dup(self, src, dst, tag):
        """dst = [src | src]: two device-to-device copies (recordable, unlike a torch copy_)."""
        half = dst.view(2, -1)
        self.add(lambda: (ops.copy_d2d(half[0], src.view(-1)), ops.copy_d2d(half[1], src.view(-1))), tag=tag)

    def groupnorm(self, x0, gamma, beta, out, *, batch, hw, c0, x1=None, c1=0, eps, silu):
        stats = self.gn_scratch(batch, hw)
        cs0, cs1, _ = self.gn_stats.consume(x0, x1, hw=hw)
        if cs0 is not None:
            self.add(lambda: ops.groupnorm_colstats(x0, gamma, beta, out, stats, cs0, batch=batch, hw=hw, c0=c0, x1=x1, c1=c1,
                                                    colstats1=cs1, eps=eps, silu=silu),
                     tag=f"groupnorm(colstats) B={batch} hw={hw} C={c0 + c1}")
        else:
            self.add(lambda: ops.groupnorm(x0, gamma, beta, out, stats, batch=batch, hw=hw, c0=c0, x1=x1, c1=c1, eps=eps, silu=silu),
                     tag=f"groupnorm B={batch} hw={hw} C={c0 + c1}")
        return out

    def layernorm(self, x, gamma, beta, out, *, rows, c, eps=1e-5):
        self.add(lambda: ops.layernorm(x, gamma, beta, out, rows=rows, c=c, eps=eps), tag=f"layernorm rows={rows} C={c}")
        return out

    def attention(self, q, k, vt, out, *, batch, heads, lq, lk, d, ldq, ldk, ldv, ldo, vt_perm16=False):
        self.add(lambda: ops.attention(q, k, vt, out, batch=batch, heads=heads, lq=lq, lk=lk, d=d, ldq=ldq, ldk=ldk, ldv=ldv,
                                       ldo=ldo, scale=d ** -0.5, vt_perm16=vt_perm16),
                 flops=4 * batch * heads * lq * lk * d, tag=f"attention B={batch} h={heads} lq={lq} lk={lk} d={d}")
        return out

    def xattn_chain(self, a, h, wo1, bo1, g2, b2, wq, k2, vt2, wo2, bo2, g3, b3, h2, n3, *, rows, rows_per_sample, lk, ldv2):
        c = 320
        self.add(lambda: ops.xattn_chain(a, h, wo1, bo1, g2, b2, wq, k2, vt2, wo2, bo2, g3, b3, h2, n3, rows=rows, rows_per_sample=rows_per_sample,
                                         lk=lk, ldv2=ldv2),
                 flops=3 * 2 * rows * c * c + 4 * rows * lk * c, tag=f"xchain rows={rows} C={c} lk={lk}", nbytes=2 * (4 * rows * c + 3 * c * c))
        return h2, n3

    def xfront(self, x, gamma, beta, wpi, bpi, g1, b1, wqk, wv, h, qk, vt, *, batch, hw, gn_eps):
        """GroupNorm table (from the producer's column sums when it left them) + the fused front of a C = 320 transformer block."""
        c = 320
        stats = self._table(x, gamma, beta, batch=batch, hw=hw, c=c, eps=gn_eps, accepts=(32,))
        rows = batch * hw
        self.add(lambda: ops.xfront(x, stats, wpi, bpi, g1, b1, wqk, wv, h, qk, vt, rows=rows, rows_per_sample=hw, ldv=vt.shape[-1]),
                 flops=4 * 2 * rows * c * c, tag=f"xfront rows={rows} C={c}", nbytes=2 * (5 * rows * c + 4 * c * c))
        return h, qk, vt

    def xtail(self, n3, h2, x, w1, b1, w2, b2, wpo, bpo, out, *, rows):
        c = 320
        cs = self.gn_stats.produce(out, "xtail", rows=rows, n=c)         # the next GroupNorm takes its statistics from these column sums
        self.add(lambda: ops.xtail(n3, h2, x, w1, b1, w2, b2, wpo, bpo, out, cs, rows=rows),
                 flops=2 * rows * c * (8 * c + 4 * c + c), tag=f"xtail rows={rows} C={c}", nbytes=2 * (4 * rows * c + 13 * c * c))
        return out

    def gn_silu_conv3x3_small_n(self, x, gamma, beta, w, bias, out, *, batch, h, w_, c, n, eps, silu=True):
        """GroupNorm (+ SiLU) -> 3x3 convolution with n <= 4 output channels in one pass over x: only the per-(sample, channel) affine
        table is computed (statistics from the producer's column sums when it left them), the normalised tensor is never written."""
        hw = h * w_
        stats = self._table(x, gamma, beta, batch=batch, hw=hw, c=c, eps=eps)
        self.add(lambda: ops.conv3x3_small_n(x, w, out, batch=batch, h=h, w_=w_, c=c, n=n, bias=bias, gn_affine=stats, silu=silu,
                                             ldo=out.shape[-1]),
                 flops=2 * batch * hw * n * 9 * c, tag=f"conv3x3(small n) B={batch} {h}x{w_} C={c} n={n}", nbytes=2 * batch * hw * (c + 8))
        return out

    def _table(self, x0, gamma, beta, *, batch, hw, c, eps, x1=None, c1=0, accepts=(256, 32), from_stats_only=False):
        """The (scale, shift) table of a GroupNorm over x0 (| x1), from whatever column sums the producers left that the consumer accepts
        (32-row slots of a GEMM epilogue, per-tile slots of a halo convolution), else from a statistics pass over x0 -- or, for a consumer
        whose table launch reads column sums only (from_stats_only: sd_groupnorm_table_cat_f16), None and no launch."""
        cs0, cs1, rps = self.gn_stats.consume(x0, x1, hw=hw, accepts=accepts)
        if from_stats_only and cs0 is None:
            return None
        table = self.gn_scratch(batch, hw)
        if from_stats_only:
            fn = lambda: ops.groupnorm_table_cat(gamma, beta, table, cs0, cs1, batch=batch, hw=hw, c0=c, c1=c1, eps=eps)
        else:
            fn = lambda: ops.groupnorm_table(x0, gamma, beta, table, batch=batch, hw=hw, c0=c, eps=eps, colstats0=cs0, rows_per_slot=rps)
        self.add(fn, tag=f"groupnorm(table) B={batch} hw={hw} C={c + c1}")
        return table

    def gn_silu_conv3x3_halo(self, x, gamma, beta, w, bias, out, *, batch, h, w_, c, n, eps, silu=True, res=None, stats=False):
        """GroupNorm (+ SiLU) -> 3x3 convolution with 128 output channels as a halo-patch convolution (sd_conv3x3_halo_f16): only the
        per-(sample, channel) affine table is computed (statistics from the producer's column sums when it left them), the normalised
        tensor is never written; stats: leave the per-tile column sums of `out` for the next GroupNorm table."""
        hw = h * w_
        table = self._table(x, gamma, beta, batch=batch, hw=hw, c=c, eps=eps)
        cs = self.gn_stats.produce(out, "tile", rows=batch * hw, n=n, hw=hw, asked=stats)
        self.add(lambda: ops.conv3x3_halo(x, w, out, batch=batch, h=h, w_=w_, c=c, n=n, bias=bias, res=res, gn_affine=table, silu=silu,
                                          colstats=cs, ldo=out.shape[-1]),
                 flops=2 * batch * hw * n * 9 * c, tag=f"conv3x3(halo) B={batch} {h}x{w_} C={c} n={n}",
                 nbytes=2 * batch * hw * (c + n * (2 if res is not None else 1)) + 2 * n * 9 * c)
        return out

    def conv3x3_c3(self, x, w27, bias, out, *, batch, h, w, n, ldx=64):
        """3 -> n channels in one launch (sd_conv3x3_c3_f16): the halo patch of a 16 x 16 tile in LDS, K = 32 operands built there
        (w27: [n][ky][kx][c] padded to 32 halfs), per-tile column sums of `out` for the next GroupNorm table."""
        cs = self.gn_stats.produce(out, "tile", rows=batch * h * w, n=n, hw=h * w)
        self.add(lambda: ops.conv3x3_c3(x, w27, out, batch=batch, h=h, w=w, ldx=ldx, n=n, bias=bias, colstats=cs),
                 flops=2 * batch * h * w * n * 32, alg_flops=2 * batch * h * w * n * 27, tag=f"conv3x3(c3) B={batch} {h}x{w} n={n}",
                 nbytes=2 * batch * h * w * (4 + n))
        return out

    def attention_causal(self, q, k, v, out, *, seqs, heads, len_, d, ldq, ldk, ldv, ldo):
        self.add(lambda: ops.attention_causal(q, k, v, out, seqs=seqs, heads=heads, len_=len_, d=d, ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo,
                                              scale=d ** -0.5),
                 flops=2 * seqs * heads * len_ * (len_ + 1) * d, tag=f"attention(causal) S={seqs} h={heads} L={len_} d={d}")
        return out

    def text_embed(self, ids, tok_emb, pos_emb, out, *, seqs, len_):
        vocab, width = tok_emb.shape
        self.add(lambda: ops.text_embed(ids, tok_emb, pos_emb, out, seqs=seqs, len_=len_, vocab=vocab, n_pos=pos_emb.shape[0], width=width),
                 tag=f"text embedding S={seqs} L={len_} C={width}", nbytes=2 * 2 * seqs * len_ * width)
        return out

    def attention_wide(self, q, k, vt, out, *, batch, heads, lq, lk, d, ldq, ldk, ldv, ldo):
        self.add(lambda: ops.attention_wide(q, k, vt, out, batch=batch, heads=heads, lq=lq, lk=lk, d=d, ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo,
                                            scale=d ** -0.5),
                 flops=4 * batch * heads * lq * lk * d, tag=f"attention(wide) B={batch} h={heads} lq={lq} lk={lk} d={d}")
        return out
