"""The operators of coma_amd/csrc/seg_ops.hip over the domain their entry points accept (case tables and references: tests/seg_ref.py;
tests/test_seg_ref_host.py checks the tables on the CPU).  Per case: (a) index outputs -- selected anchors, sort order, keep lists, levels,
top-k indices and coordinates, `valid`, counts -- equal the reference exactly; float outputs are within a bound derived from a float64
restatement that uses the kernel's own fp32 geometry, the measured ratio printed; (b) nothing that had to be written is NaN /
Inf / sentinel; (c) every guard, gap column, row past a device count and unused slot keeps its sentinel bit for bit; (d) a second launch into
fresh buffers gives the same bits (seg_box_predict: the same set, its slot order comes from an atomic counter).  Every operand element the
contract says is not read is NaN, or for integer operands a value no reference could use."""
import ctypes as C
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from oracle import seg_oracle as so
from tests import domain_kit as kit
from tests import seg_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = sr.GUARD
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
ALL1 = np.uint64(0xffffffffffffffff)


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from coma_amd.seg import ops
    return ops


def dv(t, dtype=None, fill=None):
    """An operand on the device between two guards -> the view of its body."""
    t = torch.as_tensor(np.ascontiguousarray(t) if isinstance(t, np.ndarray) else t)
    t = t.to(dtype) if dtype is not None else t
    return sr.guarded(t, fill).to(DEV)[G:-G].view(t.shape)


class Out:
    """An output buffer of `init` (a CPU tensor: sentinel or the caller's prefill) between two guards."""

    def __init__(self, init, fill=None):
        self.shape, self.fill = init.shape, fill
        self.flat = sr.guarded(init, fill).to(DEV)
        self.t = self.flat[G:-G].view(init.shape)

    def cpu(self):
        flat = self.flat.cpu()
        assert sr.guards_intact(flat, self.fill), "(c) a guard of an output was written"
        return flat[G:-G].view(self.shape)


def f32_out(*shape):
    return Out(sr.sentinel(*shape))


def i32_out(*shape):
    return Out(sr.sentinel_i32(*shape), fill=-7)


def launch(what, fn):
    """Run the launches of `fn` under the kit's fault policy: a launch error ends the session's device work, a refusal fails this case
    alone."""
    with kit.device_guard(what):
        fn()


def same_bits(a, b):
    return all(torch.equal(kit.bits(x), kit.bits(y)) for x, y in zip(a, b))


def is_sentinel(t):
    return kit.bits(t) == (kit.sentinel_bits(torch.float32) if t.dtype == F32 else sr.SENT_I32 if t.dtype == I32 else sr.SENT_U8)


# ------------------------------------------------------------------ memset, pooling, resize
@pytest.mark.parametrize("nbytes,off", sr.MEMSET_CASES)
def test_memset(ops, nbytes, off):
    for value in (0x00, 0xFF):
        buf = torch.full((G + off + nbytes + G,), sr.SENT_U8, dtype=U8, device=DEV)
        launch("seg_memset", lambda: ops.memset(buf[G + off:G + off + nbytes], value))
        got = buf.cpu()
        assert bool((got[G + off:G + off + nbytes] == value).all()), (nbytes, off, value)
        assert bool((got[:G + off] == sr.SENT_U8).all()) and bool((got[G + off + nbytes:] == sr.SENT_U8).all()), "(c) bytes outside the range were written"


@pytest.mark.parametrize("h,w,c", sr.POOL_CASES)
def test_pooling(ops, h, w, c):
    x = sr.make_pool_input(h, w, c)
    xd = dv(x.permute(0, 2, 3, 1))
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    for fn, ref in ((ops.maxpool3x3s2, F.max_pool2d(x, 3, 2, 1)), (ops.subsample2, F.max_pool2d(x, 1, 2, 0))):
        res = []
        for _ in range(2):
            out = f32_out(3, oh, ow, c)
            launch(fn.__name__, lambda: fn(xd, out.t, batch=3, h=h, w=w, c=c))
            res.append(out.cpu())
        assert torch.equal(res[0].permute(0, 3, 1, 2), ref) and not bool(res[0].isnan().any()), fn.__name__      # exact; -inf windows stay -inf
        assert same_bits(res[:1], res[1:])


@pytest.mark.parametrize("case", sr.RESIZE_CASES, ids=lambda c: c[0])
def test_resize_normalize(ops, case):
    cid, h, w, nh, nw, ph, pw, with_resized = case
    img = sr.make_resize_input(cid, h, w)
    bx, kx = so.bilinear_coeffs(w, nw)
    by, ky = so.bilinear_coeffs(h, nh)
    res = []
    for _ in range(2):
        tmp, rz, out = Out(torch.full((2, h, nw, 3), sr.SENT_U8, dtype=U8)), Out(torch.full((2, nh, nw, 3), sr.SENT_U8, dtype=U8)), f32_out(2, ph, pw, 4)
        launch(cid, lambda: ops.resize_normalize(dv(img), tmp.t, out.t, batch=2, h=h, w=w, new_h=nh, new_w=nw, pad_h=ph, pad_w=pw, bounds_x=dv(bx),
                                                 kk_x=dv(kx), bounds_y=dv(by), kk_y=dv(ky), mean=sr.RESIZE_MEAN, resized=rz.t if with_resized else None))
        res.append((tmp.cpu(), rz.cpu(), out.cpu()))
    _, rz, out = res[0]
    assert same_bits(res[0], res[1])
    mean = torch.tensor(sr.RESIZE_MEAN, dtype=F32)
    for b in range(2):
        pil = np.asarray(Image.fromarray(img[b]).resize((nw, nh), Image.BILINEAR))
        # Pillow skips a pass whose size does not change; the device always runs both with the identity table of that axis
        assert np.array_equal(pil, so.resize_bilinear_u8_ref(img[b], nh, nw))
        if with_resized:
            assert np.array_equal(rz[b].numpy(), pil)
        assert torch.equal(out[b, :nh, :nw, :3], torch.from_numpy(pil.astype(np.float32)) - mean)
    assert float(out[..., 3].abs().max()) == 0.0 and float(out[:, nh:].abs().max() if ph > nh else 0.0) == 0.0
    assert float(out[:, :, nw:].abs().max() if pw > nw else 0.0) == 0.0                                  # the pad region is exactly zero
    if not with_resized:
        assert bool(is_sentinel(rz).all())


def test_resize_normalize_is_the_oracles_preprocess(ops):
    """A 16 x 12 picture through DefaultPredictor's own sizes (shortest edge 800: a 66-fold up-scale) against so.preprocess."""
    img = sr.make_resize_input("preprocess", 16, 12)
    nh, nw = so.shortest_edge_size(16, 12)
    ph, pw = -(-nh // 32) * 32, -(-nw // 32) * 32
    bx, kx = so.bilinear_coeffs(12, nw)
    by, ky = so.bilinear_coeffs(16, nh)
    tmp, out = Out(torch.zeros(2, 16, nw, 3, dtype=U8)), f32_out(2, ph, pw, 4)
    launch("preprocess", lambda: ops.resize_normalize(dv(img), tmp.t, out.t, batch=2, h=16, w=12, new_h=nh, new_w=nw, pad_h=ph, pad_w=pw, bounds_x=dv(bx),
                                                      kk_x=dv(kx), bounds_y=dv(by), kk_y=dv(ky), mean=sr.RESIZE_MEAN))
    x, size = so.preprocess(img)
    got = out.cpu()
    assert size == (nh, nw) and torch.equal(got[..., :3].permute(0, 3, 1, 2), x) and float(got[..., 3].abs().max()) == 0.0


# ------------------------------------------------------------------ RPN selection
def _rpn_run(ops, c, preds_d, cells_d, mode):
    """mode: "levels" | "levels+scratch" | "single" -> (keys u64 [B, cap], boxes, group) on the CPU."""
    B = c.batch
    keys = Out(torch.full((B, c.cap), -1, dtype=I64), fill=0x5A5A5A5A)
    boxes, group = f32_out(B, c.cap, 4), i32_out(B, c.cap)
    kw = dict(ld=c.ld, batch=B, pre_topk=c.pre_topk, img_h=c.img[0], img_w=c.img[1], cap=c.cap)

    def go():
        if mode == "single":
            off = base = 0
            for l, (fh, fw) in enumerate(c.dims):
                ops.rpn_select(preds_d[l], cells_d[l], keys.t, boxes.t, group.t, fh=fh, fw=fw, stride=4 << l, level=l, anchor_base=base, cand_offset=off, **kw)
                off, base = off + c.takes[l], base + c.counts[l]
        else:
            scratch = Out(sr.sentinel_i32(B, sum(c.counts)), fill=-7) if mode == "levels+scratch" else None
            ops.rpn_select_levels(preds_d, cells_d, keys.t, boxes.t, group.t, dims=list(c.dims), first_stride=4, key_scratch=None if scratch is None else scratch.t,
                                  **kw)
            if scratch is not None:
                torch.cuda.synchronize()
                scratch.cpu()                                  # its guards
    launch(f"rpn {c.id} {mode}", go)
    return keys.cpu().numpy().view(np.uint64), boxes.cpu(), group.cpu()


@pytest.mark.parametrize("case", sr.RPN_CASES, ids=lambda c: c.id)
def test_rpn_select(ops, case):
    c = case
    preds = sr.make_rpn_preds(c)
    ref = sr.rpn_reference(c, preds)
    preds_d = [dv(p) for p in preds]
    cells_d = [dv(so.cell_anchors(sr.RPN_SIZES[l])) for l in range(len(c.dims))]
    runs = {m: _rpn_run(ops, c, preds_d, cells_d, m) for m in ("levels", "levels+scratch", "single")}
    keys, boxes, group = runs["levels"]
    again = _rpn_run(ops, c, preds_d, cells_d, "levels")
    worst = 0.0
    for b in range(c.batch):
        off = base = 0
        for l, r in enumerate(ref[b]):
            k = c.takes[l]
            ks = keys[b, off:off + k]
            live = ks != ALL1
            low = (ks[live] & np.uint64(0xffffffff)).astype(np.int64) - base
            want = r["sel"][r["ok"]].numpy()
            assert np.array_equal(np.sort(low), want), f"(a) image {b} level {l}: selected anchors"
            assert int((~live).sum()) == int((~r["ok"]).sum())
            assert bool((group[b, off:off + k] == l).all())
            pos = {int(a): i for i, a in enumerate(low)}
            slots = np.nonzero(live)[0]
            sel = torch.as_tensor([off + slots[pos[int(a)]] for a in want], dtype=I64)
            if len(sel):
                gb, rb = boxes[b, sel], r["boxes"][r["ok"]]
                assert bool(torch.isfinite(gb).all()), "(b)"
                worst = max(worst, float((gb - rb).abs().max()))
                # the score half of the key is the logit's order bits
                sc = r["scores"][r["ok"]].numpy()
                assert np.array_equal(ks[live][[pos[int(a)] for a in want]] >> np.uint64(32), sr.desc_keys(sc, np.zeros(len(sc))).view(np.uint64) >> np.uint64(32))
            off, base = off + k, base + c.counts[l]
        assert bool((keys[b, off:] == ALL1).all()), "(c) unused key slots keep ~0"
        assert bool(is_sentinel(boxes[b, off:]).all()) and bool(is_sentinel(group[b, off:]).all()), "(c) slots behind the last level"
    print(f"SEG_DOMAIN rpn_select {c.id}: decoded boxes max |diff| = {worst:.3e} (tolerance 1e-3)")
    assert worst <= 1e-3
    for m in ("levels+scratch", "single"):                        # the three forms give the same candidate list, bit for bit
        assert np.array_equal(runs[m][0], keys) and same_bits(runs[m][1:], (boxes, group)), m
    assert np.array_equal(again[0], keys) and same_bits(again[1:], (boxes, group)), "(d)"


# ------------------------------------------------------------------ sort, NMS
@pytest.mark.parametrize("cap", sr.SORT_CAPS)
def test_sort_candidates(ops, cap):
    keys, boxes, group, scores, orders = sr.make_sort_inputs(cap)
    B = len(orders)
    kd, bd, gd = dv(keys, fill=0x5A5A5A5A), dv(boxes), dv(group, fill=-7)
    res = []
    for _ in range(2):
        o = [f32_out(B, cap, 4), f32_out(B, cap), i32_out(B, cap), i32_out(B, cap), i32_out(B)]
        launch(f"sort cap={cap}", lambda: ops.sort_candidates(kd, bd, gd, *[x.t for x in o], batch=B, cap=cap))
        res.append([x.cpu() for x in o])
    sb, ss, sg, ssrc, nv = res[0]
    assert same_bits(res[0], res[1]), "(d)"
    for b, order in enumerate(orders):
        n = len(order)
        assert int(nv[b]) == n, (b, int(nv[b]), n)
        assert np.array_equal(ssrc[b, :n].numpy(), order * 3 + 1), f"(a) image {b}: order"
        assert np.array_equal(kit.bits(ss[b, :n]).numpy(), scores[b, order].view(np.int32)) and np.array_equal(sg[b, :n].numpy(), group[b, order])
        assert np.array_equal(sb[b, :n].numpy(), boxes[b, order])
        assert bool((sb[b, n:] == 0).all()) and bool((kit.bits(ss[b, n:]) == 0).all()) and bool((sg[b, n:] == -1).all()) and bool((ssrc[b, n:] == -1).all())


@pytest.mark.parametrize("case", sr.NMS_CASES, ids=lambda c: c.id)
def test_nms(ops, case):
    c = case
    boxes, scores, group, src = sr.make_nms_inputs(c)
    B, K = len(c.n), c.max_keep
    ins = [dv(boxes), dv(scores), dv(group, fill=-7), dv(src, fill=-7), dv(np.asarray(c.n, np.int32), fill=-7)]
    res = []
    for _ in range(2):
        ws = Out(torch.full((B, c.cap, c.cap // 64), -1, dtype=I64), fill=0x5A5A5A5A)          # every bit set: a word read before it was written suppresses
        o = [i32_out(B, K), f32_out(B, K, 4), f32_out(B, K), i32_out(B, K), i32_out(B, K), i32_out(B)]
        launch(f"nms {c.id}", lambda: ops.nms(*ins, ws.t, *[x.t for x in o], batch=B, cap=c.cap, thresh=c.thresh, max_keep=K))
        ws.cpu()
        res.append([x.cpu() for x in o])
    kp, ob, osc, og, osrc, oc = res[0]
    assert same_bits(res[0], res[1]), "(d)"
    for b in range(B):
        keep = sr.nms_reference(c, boxes, scores, group, b)
        m = len(keep)
        assert int(oc[b]) == m, (b, int(oc[b]), m)
        assert np.array_equal(kp[b, :m].numpy(), keep), f"(a) image {b}: keep list"
        assert np.array_equal(ob[b, :m].numpy(), boxes[b, keep]) and np.array_equal(osc[b, :m].numpy(), scores[b, keep])
        assert np.array_equal(og[b, :m].numpy(), group[b, keep]) and np.array_equal(osrc[b, :m].numpy(), src[b, keep])
        assert bool((kp[b, m:] == -1).all()) and bool((ob[b, m:] == 0).all()) and bool((osc[b, m:] == 0).all()) and bool((og[b, m:] == -1).all()) \
            and bool((osrc[b, m:] == -1).all())
    if c.kind == "dyadic":                                        # the construction does hit the threshold: pairs at IoU 0.5 exactly, both kept
        keep = set(sr.nms_reference(c, boxes, scores, group, 0).tolist())
        bx, hit = boxes[0, :c.n[0]], 0
        for i in keep:
            for j in keep:
                if i < j and group[0, i] == group[0, j]:
                    iw, ih = min(bx[i, 2], bx[j, 2]) - max(bx[i, 0], bx[j, 0]), min(bx[i, 3], bx[j, 3]) - max(bx[i, 1], bx[j, 1])
                    ai, aj = (bx[i, 2] - bx[i, 0]) * (bx[i, 3] - bx[i, 1]), (bx[j, 2] - bx[j, 0]) * (bx[j, 3] - bx[j, 1])
                    hit += iw > 0 and ih > 0 and iw * ih * 2 == ai + aj - iw * ih
        assert hit > 0


# ------------------------------------------------------------------ ROIAlign
@pytest.mark.parametrize("case", sr.ROI_CASES, ids=lambda c: c.id)
def test_roi_align(ops, case):
    c = case
    feats, boxes = sr.make_roi_inputs(c)
    B, S = len(c.counts), c.out_size
    fd = [dv(f.permute(0, 2, 3, 1)) for f in feats]
    bd, cd = dv(boxes), dv(np.asarray(c.counts, np.int32), fill=-7)
    res = []
    for _ in range(2):
        out, lv = f32_out(B * c.R, S * S * c.c), i32_out(B * c.R)
        launch(f"roi_align {c.id}", lambda: ops.roi_align(fd, bd, cd, out.t, lv.t, h2=c.h2, w2=c.w2, c=c.c, batch=B, R=c.R, out_size=S))
        res.append((out.cpu(), lv.cpu()))
    out, lv = res[0]
    assert same_bits(res[0], res[1]), "(d)"
    o = out.view(B, c.R, S, S, c.c).permute(0, 1, 4, 2, 3)
    lv = lv.view(B, c.R)
    worst, worst_rel = 0.0, 0.0
    for b, n in enumerate(c.counts):
        bb = torch.from_numpy(boxes[b, :n])
        want = sr.roi_levels_reference(bb)
        assert torch.equal(lv[b, :n].long(), want), f"(a) image {b}: levels {lv[b, :n].tolist()} != {want.tolist()}"
        assert bool(is_sentinel(lv[b, n:]).all()) and bool(is_sentinel(out.view(B, c.R, -1)[b, n:]).all()), "(c) rows past the count"
        assert bool(torch.isfinite(o[b, :n]).all()), "(b)"
        for i in range(n):
            l = int(want[i])
            ref, mag, samples = sr.roi_align_reference64(feats[l][b], boxes[b, i], S, 1.0 / (4 << l))
            err = (o[b, i].double() - ref).abs()
            if samples == 0:
                assert float(err.max()) == 0.0, f"image {b} roi {i}: a box without samples pools zeros"
                continue
            bound = sr.roi_bound(samples, mag)
            worst = max(worst, float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0)
            assert bool((err <= bound).all()), f"(a) image {b} roi {i} (level {l}, {samples} samples): {float((err / bound.clamp_min(1e-300)).max()):.3f} x the bound"
            area = (bb[i, 2] - bb[i, 0]) * (bb[i, 3] - bb[i, 1])
            if float(area) > 0:                                    # the looser check against the oracle itself
                oref = so.roi_align_ref(feats[l][b], bb[i:i + 1], S, 1.0 / (4 << l))[0]
                worst_rel = max(worst_rel, float((o[b, i] - oref).abs().max() / (oref.abs().max() + 1e-30)))
    print(f"SEG_DOMAIN roi_align {c.id}: worst |err| / bound = {worst:.3f}; against the oracle rel {worst_rel:.2e} (<= 1e-5)")
    assert worst_rel <= 1e-5


# ------------------------------------------------------------------ box predictor, detections
@pytest.mark.parametrize("case", sr.BOXPRED_CASES, ids=lambda c: c.id)
def test_box_predict(ops, case):
    c = case
    pred, props = sr.make_boxpred_inputs(c)
    B = len(c.counts)
    pd, prd, cd = dv(pred), dv(props), dv(np.asarray(c.counts, np.int32), fill=-7)
    res = []
    for _ in range(2):
        keys = Out(torch.full((B, c.cap), -1, dtype=I64), fill=0x5A5A5A5A)
        o = [f32_out(B, c.cap, 4), i32_out(B, c.cap), Out(torch.zeros(B, dtype=I32), fill=-7), f32_out(B * c.R, 81)]
        launch(f"box_predict {c.id}", lambda: ops.box_predict(pd, prd, cd, keys.t, o[0].t, o[1].t, o[2].t, o[3].t, ld=c.ld, batch=B, R=c.R, img_h=c.img[0],
                                                              img_w=c.img[1], score_thresh=c.thresh, cap=c.cap))
        res.append([keys.cpu()] + [x.cpu() for x in o])
    worst = 0.0
    for b, n in enumerate(c.counts):
        ref = sr.boxpred_reference(c, pred, props, b)
        exact_rows = (0,) if b == 0 else ()
        border = sr.boxpred_border(c, ref, exact_rows)
        ref_low = (ref["cand_inds"][:, 0] * 80 + ref["cand_inds"][:, 1]).tolist()
        sets = []
        for keys, cb, cg, cn, probs in res:
            total = int(cn[b])
            stored = min(total, c.cap)
            ks = keys[b].numpy().view(np.uint64)
            low = (ks[:stored] & np.uint64(0xffffffff)).astype(np.int64).tolist()
            assert len(set(low)) == stored and bool((ks[stored:] == ALL1).all()), "(c) nothing behind the stored candidates"
            assert bool(is_sentinel(cb[b, stored:]).all()) and bool(is_sentinel(cg[b, stored:]).all())
            if total <= c.cap:
                assert set(low) - border == set(ref_low) - border, f"(a) image {b}: candidates"
            else:
                assert set(low) <= set(ref_low) | border, f"(a) image {b}: stored candidates are a subset of the oracle's"
            assert abs(total - len(ref_low)) <= len(border) and (border or total == len(ref_low)), f"cand_count {total} vs {len(ref_low)}"
            pos = {v: i for i, v in enumerate(ref_low)}
            for s, v in enumerate(low):
                if v in pos:
                    worst = max(worst, float((cb[b, s] - ref["cand_boxes"][pos[v]]).abs().max()))
                    assert int(cg[b, s]) == v % 80
                    own = probs.view(B, c.R, 81)[b, v // 80, v % 80:v % 80 + 1].numpy()                  # the score word: the device's own probability
                    assert sr.desc_keys(own, [0]).view(np.uint64)[0] >> np.uint64(32) == ks[s] >> np.uint64(32)
            got_p = probs.view(B, c.R, 81)[b]
            if n:
                fin = torch.isfinite(ref["probs"]).all(dim=1)
                assert float((got_p[:n][fin] - ref["probs"][fin]).abs().max() / ref["probs"][fin].abs().max()) <= 1e-5
                assert bool(got_p[:n][~fin].isnan().all())
            assert bool(is_sentinel(got_p[n:]).all()), "(c) probability rows past the count"
            sets.append({(v, tuple(kit.bits(cb[b, s]).tolist()), int(ks[s] >> np.uint64(32))) for s, v in enumerate(low)})
            if b == 0 and n:
                assert not any(v // 80 in (0, 1) for v in low), "rows 0 (every probability AT the threshold) and 1 (an infinite logit) give no candidate"
        if int(res[0][3][b]) <= c.cap:
            assert sets[0] == sets[1], "(d) the second launch gives another candidate set"
        assert int(res[0][3][b]) == int(res[1][3][b])
    print(f"SEG_DOMAIN box_predict {c.id}: decoded boxes max |diff| = {worst:.3e} (tolerance 2e-3)")
    assert worst <= 2e-3


def test_finalize_detections(ops):
    """Scale + clip + nonempty: boxes that empty after the clip, NaN kept as NaN, rows past the count zero."""
    B, R, counts = 2, 6, (6, 2)
    det = np.full((B, R, 4), np.nan, np.float32)
    det[0] = [[10, 20, 300, 400], [900, 10, 950, 60], [100, 810, 200, 900], [5, 5, 5.001, 90], [np.nan, 10, 50, 60], [-30, -40, 20, 30]]
    det[1, :2] = [[0, 0, 800, 800], [400, 400, 400, 500]]
    res = []
    for _ in range(2):
        ob, valid = f32_out(B, R, 4), i32_out(B, R)
        launch("finalize", lambda: ops.finalize_detections(dv(det), dv(np.asarray(counts, np.int32), fill=-7), ob.t, valid.t, batch=B, R=R, img_h=800.0,
                                                           img_w=760.0, out_h=96, out_w=128))
        res.append((ob.cpu(), valid.cpu()))
    ob, valid = res[0]
    assert same_bits(res[0], res[1])
    for b, n in enumerate(counts):
        bb = torch.from_numpy(det[b, :n]).clone()
        bb[:, 0::2] *= torch.tensor(np.float32(128) / np.float32(760))             # the scale as the entry point forms it: one fp32 division
        bb[:, 1::2] *= torch.tensor(np.float32(96) / np.float32(800))
        bb = so.clip_boxes(bb, 96, 128)
        ne = ((bb[:, 2] - bb[:, 0]) > 0) & ((bb[:, 3] - bb[:, 1]) > 0)
        assert torch.equal(ob[b, :n].isnan(), bb.isnan()) and torch.equal(kit.bits(ob[b, :n].nan_to_num(7.0)), kit.bits(bb.nan_to_num(7.0)))
        assert torch.equal(valid[b, :n].bool(), ne)
        assert bool((kit.bits(ob[b, n:]) == 0).all()) and bool((valid[b, n:] == 0).all())
    assert valid[0].tolist() == [1, 0, 0, 1, 0, 1] and bool(ob[0, 4, 0].isnan())


# ------------------------------------------------------------------ PointRend pieces
@pytest.mark.parametrize("case", sr.SAMPLE_CASES, ids=lambda c: c.id)
def test_point_sample(ops, case):
    c = case
    feat, boxes, coords = sr.make_sample_inputs(c)
    B = len(c.counts)
    rois, ldo = B * c.R, c.ldo or c.c
    stride = rois * c.P * ldo + c.gap
    fd, cd = dv(feat.permute(0, 2, 3, 1)), dv(np.asarray(c.counts, np.int32), fill=-7)
    bd, xy = None if boxes is None else dv(boxes), None if coords is None else dv(coords)
    res = []
    for _ in range(2):
        out = f32_out(c.n_copies * stride)
        launch(f"point_sample {c.id}", lambda: ops.point_sample(fd, out.t, fh=c.fh, fw=c.fw, c=c.c, per_roi=c.per_roi, feat_scale=0.25 if not c.per_roi else 1.0,
                                                                boxes=bd, count=cd, batch=B, R=c.R, coords=xy, P=c.P, grid_side=int(round(c.P ** 0.5)) if c.grid else 0,
                                                                ldo=ldo, col0=c.col0, n_copies=c.n_copies, copy_stride=stride))
        res.append(out.cpu())
    out = res[0]
    assert torch.equal(kit.bits(out), kit.bits(res[1])), "(d)"
    cc = sr.sample_coords(c, coords, rois)
    worst, worst_rel = 0.0, 0.0
    written = torch.zeros(c.n_copies * stride, dtype=torch.bool)
    for k in range(c.n_copies):
        blk = out[k * stride:k * stride + rois * c.P * ldo].view(rois, c.P, ldo)
        wm = written[k * stride:k * stride + rois * c.P * ldo].view(rois, c.P, ldo)
        for b, n in enumerate(c.counts):
            for i in range(n):
                r = b * c.R + i
                ref, mag = sr.point_sample_reference64(c, feat[r if c.per_roi else b], None if boxes is None else boxes[b, i], cc[r])
                got = blk[r, :, c.col0:c.col0 + c.c]
                wm[r, :, c.col0:c.col0 + c.c] = True
                assert bool(torch.isfinite(got).all()), "(b)"
                err, bound = (got.double() - ref).abs(), sr.gamma(6) * mag
                worst = max(worst, float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0)
                assert bool((err <= bound).all()), f"(a) roi {r} copy {k}: {float((err / bound.clamp_min(1e-300)).max()):.3f} x the bound"
                if c.per_roi:
                    oref = so.point_sample(feat[r:r + 1], cc[r:r + 1])[0].t()
                else:
                    oref = so.fine_features(feat[b:b + 1], torch.from_numpy(boxes[b, i:i + 1]), cc[r:r + 1].clone())[0].t()
                worst_rel = max(worst_rel, float((got - oref).abs().max() / (oref.abs().max() + 1e-30)))
    assert bool(is_sentinel(out[~written]).all()), "(c) guard columns, rows past the count or the gap between copies were written"
    print(f"SEG_DOMAIN point_sample {c.id}: worst |err| / bound = {worst:.3f}; against the oracle rel {worst_rel:.2e} (<= 1e-5)")
    assert worst_rel <= 1e-5


@pytest.mark.parametrize("s", sr.UPSAMPLE_SIDES)
def test_upsample2x(ops, s):
    B, R, counts = 2, 3, (3, 1)
    m = torch.randn(B * R, s, s, generator=sr.gen_of(f"up-{s}"))
    m[4:] = sr.NAN
    res = []
    for _ in range(2):
        out = f32_out(B * R, 2 * s, 2 * s)
        launch(f"upsample2x s={s}", lambda: ops.upsample2x(dv(m), dv(np.asarray(counts, np.int32), fill=-7), out.t, batch=B, R=R, s=s))
        res.append(out.cpu())
    out = res[0]
    assert torch.equal(kit.bits(out), kit.bits(res[1]))
    ref = F.interpolate(m[:4, None].double(), scale_factor=2, mode="bilinear", align_corners=False)[:, 0]
    mag = F.interpolate(m[:4, None].double().abs(), scale_factor=2, mode="bilinear", align_corners=False)[:, 0]
    err = (out[:4].double() - ref).abs()
    # the weights 0.25 / 0.75 and their products are exact in fp32: four products and three sums, nested -- at most 5 roundings on a term
    ratio = float((err / (sr.gamma(5) * mag)).max())
    print(f"SEG_DOMAIN upsample2x s={s}: worst |err| / bound = {ratio:.3f}")
    assert bool(torch.isfinite(out[:4]).all()) and ratio <= 1.0 and bool(is_sentinel(out[4:]).all())


@pytest.mark.parametrize("s,k", sr.TOPK_CASES)
def test_topk_points(ops, s, k):
    m = sr.make_topk_maps(s, k)
    R = len(sr.TOPK_KINDS)
    md = dv(torch.cat([m[:R - 1], torch.full((1, s, s), sr.NAN)]))
    res = []
    for _ in range(2):
        idx, crd = i32_out(R, k), f32_out(R, k, 2)
        launch(f"topk_points s={s} k={k}", lambda: ops.topk_points(md, dv(np.asarray([R - 1], np.int32), fill=-7), idx.t, crd.t, batch=1, R=R, s=s, k=k))
        res.append((idx.cpu(), crd.cpu()))
    idx, crd = res[0]
    assert same_bits(res[0], res[1])
    for r, kind in enumerate(sr.TOPK_KINDS[:-1]):
        want, wc = sr.topk_reference(m[r], k)
        assert torch.equal(idx[r].long(), want), f"(a) {kind}: indices"
        assert torch.equal(kit.bits(crd[r]), kit.bits(wc)), f"(a) {kind}: coordinates"
    assert bool(is_sentinel(idx[R - 1]).all()) and bool(is_sentinel(crd[R - 1]).all()), "(c) the map past the count"


@pytest.mark.parametrize("kdim,ldx,s,with_idx", sr.LOGIT_CASES)
def test_point_logit_scatter(ops, kdim, ldx, s, with_idx):
    B, R, counts = 2, 3, (2, 3)
    g = sr.gen_of(f"logit-{kdim}-{ldx}-{s}")
    P = 5 if with_idx else s * s
    x = torch.full((B * R * P, ldx), sr.NAN)
    x[:, :kdim] = torch.randn(B * R * P, kdim, generator=g)
    w, bias = torch.randn(80, kdim, generator=g) / kdim ** 0.5, torch.randn(80, generator=g)
    classes = torch.randint(0, 80, (B * R,), generator=g).to(I32)
    idx = torch.stack([torch.randperm(s * s, generator=g)[:P] for _ in range(B * R)]).to(I32) if with_idx else None
    x[2 * P:3 * P] = sr.NAN                                        # roi 2 lies past image 0's count
    classes[2] = -1
    if idx is not None:
        idx[2] = 1 << 30
    before = torch.randn(B * R, s * s, generator=g)
    res = []
    for _ in range(2):
        mp = Out(before.clone())
        launch(f"point_logit kdim={kdim}", lambda: ops.point_logit_scatter(dv(x), dv(w), dv(bias), dv(classes, fill=-7), dv(np.asarray(counts, np.int32), fill=-7),
                                                                           mp.t, None if idx is None else dv(idx, fill=-7), ldx=ldx, kdim=kdim, batch=B, R=R, P=P,
                                                                           s=s))
        res.append(mp.cpu())
    got = res[0]
    assert torch.equal(kit.bits(got), kit.bits(res[1]))
    worst = 0.0
    for r in range(B * R):
        if r % R >= counts[r // R]:
            assert torch.equal(kit.bits(got[r]), kit.bits(before[r])), "(c) a map past the count"
            continue
        xs, wr = x[r * P:(r + 1) * P, :kdim].double(), w[classes[r]].double()
        ref, mag = xs @ wr + bias[classes[r]].double(), xs.abs() @ wr.abs() + bias[classes[r]].double().abs()
        where = idx[r].long() if idx is not None else torch.arange(P)
        err = (got[r][where].double() - ref).abs()
        worst = max(worst, float((err / (sr.gamma(kdim + 1) * mag)).max()))
        rest = torch.ones(s * s, dtype=torch.bool)
        rest[where] = False
        assert torch.equal(kit.bits(got[r][rest]), kit.bits(before[r][rest])), "(c) a pixel outside idx"
    print(f"SEG_DOMAIN point_logit kdim={kdim}: worst |err| / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("case", sr.PASTE_CASES, ids=lambda c: c.id)
def test_paste_masks(ops, case):
    c = case
    logits, boxes, valid, classes = sr.make_paste_inputs(c)
    B, H, W = len(c.counts), c.out_h, c.out_w
    ins = [dv(logits), dv(boxes), dv(valid, fill=-7), dv(classes, fill=-7), dv(np.asarray(c.counts, np.int32), fill=-7)]
    res = []
    for _ in range(2):
        merged, masks = Out(torch.full((B, H, W), sr.SENT_U8, dtype=U8)), Out(torch.full((B, c.R, H, W), sr.SENT_U8, dtype=U8))
        launch(f"paste {c.id}", lambda: ops.paste_masks(*ins, merged.t, masks.t if c.masks else None, s=c.s, batch=B, R=c.R, out_h=H, out_w=W, cat_id=c.cat_id))
        res.append((merged.cpu(), masks.cpu()))
    merged, masks = res[0]
    assert same_bits(res[0], res[1])
    if not c.masks:
        assert bool(is_sentinel(masks).all())
    excluded = total = 0
    for b, n in enumerate(c.counts):
        ref, p64 = sr.paste_reference(c, logits, boxes, valid, b)
        ok = torch.from_numpy(valid[b, :n]).bool()
        skip = sr.paste_excluded(p64) & ok[:, None, None]
        excluded, total = excluded + int(skip.sum()), total + n * H * W
        if c.masks:
            got = masks[b, :n].bool()
            assert bool((masks[b] <= 1).all()) and torch.equal(got[~skip], ref[~skip]), f"(a) image {b}: {int((got != ref)[~skip].sum())} pixels differ"
            assert not bool(masks[b, n:].any()), "rows past the count are pasted empty"
        own = torch.from_numpy(classes[b, :n] == c.cat_id)[:, None, None]
        person, unsure = (ref & own).any(0), (skip & own).any(0)
        assert torch.equal(merged[b].bool()[~unsure], person[~unsure]) and bool((merged[b] <= 1).all()), f"(a) image {b}: merged mask"
    print(f"SEG_DOMAIN paste {c.id}: {excluded} of {total} pixels within 1e-5 of 0.5 (not compared; cap 1 %)")
    assert excluded <= 0.01 * max(total, 1)


# ------------------------------------------------------------------ refusals
def test_operator_refusals_are_reported_not_launched(ops, hip_lib):
    """Every row of seg_ref.OPS_REFUSALS through the real entry point with real device pointers: the error text, and the buffer every pointer
    argument names keeps its sentinel."""
    buf = sr.sentinel(1 << 16).to(DEV)
    for fn, text, args in sr.OPS_REFUSALS:
        a = [C.c_void_p(buf.data_ptr()) if v is kit.PTR else v for v in args] + [None]
        assert getattr(hip_lib, fn)(*a) == -1, (fn, args)
        msg = hip_lib.coma_last_error().decode()
        assert msg.startswith(fn + ":") and re.search(text, msg), (fn, msg)
    torch.cuda.synchronize()
    assert bool((kit.bits(buf.cpu()) == kit.sentinel_bits(torch.float32)).all())
