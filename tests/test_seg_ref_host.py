"""CPU checks of tests/seg_ref.py and of seg_conv_gemm_describe: every GEMM case reaches the launch it names and the table covers every
instantiation x {residual prefetch, split-K, row gate}; the integer family stays exact in fp32; the float64 references meet their own
bounds against torch's fp32 results (so a failure of the device tests is the device's); the refusal tables raise through the real entry
points where no launch is needed; the three level cut points of roi_align_kernel agree with the oracle's formula on every float around
them; the exclusion caps of the paste and score-threshold comparisons hold for the chosen inputs."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from coma_amd._lib import ComaHipError
from oracle import seg_oracle as so
from tests import domain_kit as kit
from tests import seg_ref as sr


@pytest.fixture(scope="module")
def ops(hip_lib):
    from coma_amd.seg import ops
    return ops


def describe(ops, c):
    t = sr.gemm_fake_tensors(c)
    return ops.conv_gemm_describe(t["x"], t["w"], t["out"], **sr.gemm_kwargs(c, t))


# ------------------------------------------------------------------ the GEMM table
def test_gemm_case_ids_are_unique_and_small():
    ids = [c.id for c in sr.GEMM_CASES]
    assert len(set(ids)) == len(ids) and 40 <= len(ids) <= 60
    for c in sr.GEMM_CASES:
        assert c.n <= 260 and c.kp <= 2304 and (c.m <= 600 or c.id == "rule-n260-m6530-nk13-t1"), c.id


@pytest.mark.parametrize("case", sr.GEMM_CASES, ids=lambda c: c.id)
def test_gemm_case_reaches_the_launch_it_names(ops, case):
    c, ch = case, describe(ops, case)
    assert (ch.tile, bool(ch.uni), bool(ch.pre), ch.splits) == (c.x_tile, c.x_uni, c.x_pre, c.x_splits), ch.asdict()
    assert (ch.bm, ch.bn, ch.nk) == (128, c.bn, c.nk) and ch.slab_elems == c.slab_elems and ch.ws_ld == -(-c.n // c.bn) * c.bn
    assert ch.grid_x == -(-c.m // 128) and ch.grid_y == -(-c.n // c.bn)
    assert ch.nk_per == -(-c.nk // min(c.split_k, c.nk)) if c.split_k > 1 else ch.nk_per * (ch.splits - 1) < c.nk <= ch.nk_per * ch.splits
    assert ch.pre == (c.res_mode != 0 and ch.splits == 1 and c.nk <= 4)


def test_gemm_table_covers_every_instantiation_and_branch():
    cs = sr.GEMM_CASES
    for tile in (1, 2, 3):
        for uni in (False, True):
            inst = [c for c in cs if (c.x_tile, c.x_uni) == (tile, uni)]
            assert any(c.x_pre for c in inst), ("PRE", tile, uni)
            assert any(not c.x_pre and c.x_splits == 1 for c in inst), ("plain", tile, uni)
        assert any(c.x_tile == tile and c.x_splits > 1 for c in cs), ("split", tile)
        assert any(c.x_tile == tile and c.gated for c in cs), ("gate", tile)
    assert any(c.x_splits > 1 and not c.x_uni for c in cs) and any(c.x_splits > 1 and c.gated for c in cs)
    assert {1, 2, 3, 4, 5, 8, 9, 72} <= {c.nk for c in cs}
    assert {c.nk for c in cs if c.x_pre} == {1, 2, 3, 4}                              # both branches of the peeled tail, and nk = 1
    assert {1, 127, 128, 129, 300} <= {c.m for c in cs} and {1, 15, 31, 33, 63, 65, 127, 129, 250} <= {c.n for c in cs}
    assert {c.tile for c in cs} == {0, 1, 2, 3} and {c.x_tile for c in cs if c.tile == 0 and c.n > 64} == {1, 2}      # both outcomes of the 128 x 64 rule
    assert {4, 12, 36, 336} <= {c.c for c in cs if not c.x_uni}
    forms = {(c.kh, c.kw, c.stride, c.pad) for c in cs}
    assert {(1, 1, 1, 0), (1, 1, 2, 0), (3, 3, 1, 1), (3, 3, 2, 1), (2, 2, 2, 0), (1, 3, 1, 0), (3, 1, 1, 0), (3, 3, 1, 2), (7, 7, 2, 3)} <= forms
    assert any(c.in_h == 1 and c.kh == 3 for c in cs) and any(c.in_w == 1 and c.kw == 3 for c in cs)
    assert any(c.stride == 2 and c.kh == 1 and c.in_h % 2 and c.in_w % 2 for c in cs)
    assert any(c.ldx > c.c for c in cs if c.x_uni) and any(c.ldx > c.c for c in cs if not c.x_uni)
    assert any(c.ldr > c.n and c.ldr % 4 for c in cs) and any(c.ldo > c.n and c.ldo % 4 for c in cs) and any(not c.bias for c in cs)
    for mode in (1, 2):
        r = [c for c in cs if c.res_mode == mode]
        vec = lambda c: c.ldo_ % 4 == 0 and c.ldr_ % 4 == 0
        assert any(c.x_pre and vec(c) for c in r), ("PRE", mode)
        assert any(not c.x_pre and c.x_splits == 1 and c.nk >= 5 and vec(c) for c in r), ("epilogue", mode)
        assert any(c.x_splits == 1 and (not vec(c) or c.n % 4) for c in r), ("tail", mode)
        assert any(c.x_splits > 1 for c in r), ("reduce", mode)
    gated = [c for c in cs if c.gated]
    assert any(sum(c.counts) == 0 for c in gated) and any(c.counts[0] * c.rows_per_item == c.unit_rows for c in gated)
    assert all(c.unit_rows == 245 for c in gated)
    # a row tile without a valid row: rows 128 .. 255 when unit 0 computes fewer than 128 rows and unit 1 none
    empty = [c for c in gated if c.counts[0] * c.rows_per_item <= 128 and c.counts[1] == 0 and sum(c.counts)]
    assert any(c.x_splits == 1 for c in empty) and any(c.x_splits > 1 for c in empty)
    assert {0, 2, 5, -1} <= {c.split_k for c in cs} and any(c.split_k > c.nk for c in cs)
    assert any(c.split_k == 0 and c.ws_slabs and c.x_splits > 1 for c in cs) and any(c.split_k == 0 and c.ws_slabs and c.x_splits == 1 for c in cs)
    assert any(c.split_k > 1 and c.nk % c.x_splits for c in cs)                      # a ragged last slice
    rule = {c.id: c for c in cs if c.split_k == 0 and c.ws_slabs}
    assert rule["split0-rule-holds-3-slabs"].x_splits == 3 < rule["split0-rule-splits8-3x3-res1"].x_splits      # fewer slabs than the rule asks for


@pytest.mark.parametrize("case", sr.GEMM_CASES, ids=lambda c: c.id)
def test_gemm_references(case):
    """The integer family is exact in fp32 (every partial sum below 2^24: the float64 reference is an integer of that size and torch's fp32
    result equals it), and torch's fp32 result of the normal family is within the bound of the float64 reference."""
    c = case
    inp = sr.make_gemm_inputs(c, "int")
    assert sr.gemm_int_peak(c, inp) < 2 ** 24
    ref, _ = sr.gemm_reference(c, inp)
    valid = sr.gemm_valid_rows(c)
    assert bool((ref == ref.round()).all()) and torch.equal(sr.gemm_reference(c, inp, torch.float32)[0][valid].double(), ref[valid])
    for t in (inp.x[..., :c.c], inp.w, inp.bias, None if inp.res is None else inp.res[:, :c.n]):
        assert t is None or float(t.nan_to_num(0.0).abs().max()) <= 4.0
    inp = sr.make_gemm_inputs(c, "normal")
    ref, mag = sr.gemm_reference(c, inp)
    cpu32 = sr.gemm_reference(c, inp, torch.float32)[0].double()
    ratio = float(((cpu32 - ref).abs() / sr.gemm_bound(c, mag))[valid].max()) if bool(valid.any()) else 0.0
    print(f"SEG_DOMAIN gemm {c.id} family=normal cpu fp32 worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    # what is not read is NaN, what is written is a prefix of the units
    if c.ldx_ > c.c:
        assert bool(inp.x[..., c.c:].isnan().all())
    if c.gated:
        assert bool(inp.x[~valid].isnan().all()) and bool(sr.gemm_written_mask(c)[valid, :c.n].all()) and not bool(sr.gemm_written_mask(c)[~valid].any())


def test_gemm_refusals_raise_through_describe(ops, hip_lib):
    for text, change in sr.GEMM_REFUSALS:
        kw = {k: (4096 if v is kit.PTR else v) for k, v in {**sr.GEMM_REFUSAL_BASE, **change}.items()}
        x, w, out = kw.pop("x"), kw.pop("w"), kw.pop("out")
        with pytest.raises(ComaHipError, match=r"seg_conv_gemm_describe failed \(-1\): seg_conv_gemm_f32: .*" + text):
            ops.conv_gemm_describe(x, w, out, **kw)
    kw = {k: (4096 if v is kit.PTR else v) for k, v in sr.GEMM_REFUSAL_BASE.items()}
    x, w, out = kw.pop("x"), kw.pop("w"), kw.pop("out")
    assert ops.conv_gemm_describe(x, w, out, **kw).tile == 3                         # the base row itself is accepted
    ch = ops.SegConvChoice()
    assert hip_lib.seg_conv_gemm_describe(None, C.byref(ch)) == -1 and b"seg_conv_gemm_f32: null descriptor" in hip_lib.coma_last_error()
    d = ops.SegConvDesc()
    assert hip_lib.seg_conv_gemm_describe(C.byref(d), None) == -1 and b"null choice" in hip_lib.coma_last_error()
    assert hip_lib.seg_conv_gemm_f32(None, None) == -1 and b"null descriptor" in hip_lib.coma_last_error()


# ------------------------------------------------------------------ level assignment
@pytest.mark.parametrize("k", range(3))
def test_level_cuts_agree_with_assign_levels_around_each_cut(k):
    """For every float within 8 floats of each cut (and of the power of two it sits under), the three comparisons give the level of the
    oracle's formula -- evaluated as assign_levels evaluates it, on whole tensors and one element at a time."""
    cut, power = sr.LEVEL_CUTS[k], (0.5, 1.0, 2.0)[k]
    assert np.float32(cut) == cut and cut < power and (power - cut) / power < 4 * 2.0 ** -23
    v = torch.from_numpy(np.unique(np.concatenate([sr.floats_around(cut, 8), sr.floats_around(power, 8)])))
    want = sr.level_by_formula(v)
    assert torch.equal(sr.level_by_cuts(v), want)
    assert torch.equal(torch.cat([sr.level_by_formula(v[i:i + 1]) for i in range(len(v))]), want)
    i = int((v == np.float32(cut)).nonzero()[0])
    assert int(want[i]) == k + 1 and int(want[i - 1]) == k                           # the cut is the smallest float of its level


def test_level_cuts_on_the_boundary_boxes():
    """The 54 boxes with sides on and up to 4 floats either side of 112, 224 and 448: the cut rule on the kernel's v equals assign_levels,
    and the literals 0.5, 1, 2 the kernel used before do not (16 of the 54)."""
    boxes = sr.level_boundary_boxes()
    assert boxes.shape == (54, 4)
    v = torch.sqrt((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])) / 224 + 1e-8
    want = so.assign_levels(boxes)
    assert torch.equal(sr.level_by_cuts(v), want)
    old = (v >= 0.5).long() + (v >= 1.0).long() + (v >= 2.0).long()
    assert int((old != want).sum()) == 16
    g = torch.Generator().manual_seed(0)
    b = torch.rand(200000, 4, generator=g) * 800
    b[:, 2:] += b[:, :2]
    assert torch.equal(sr.level_by_cuts(torch.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) / 224 + 1e-8), so.assign_levels(b))


# ------------------------------------------------------------------ the operator tables
def test_operator_refusals_raise_before_any_launch(hip_lib):
    """seg_ref.OPS_REFUSALS through the real entry points with addresses that are never dereferenced: refused by the argument checks."""
    assert {fn for fn, _, _ in sr.OPS_REFUSALS} >= {"seg_memset", "seg_maxpool3x3s2_f32", "seg_subsample2_f32", "seg_resize_normalize_u8", "seg_rpn_select",
                                                     "seg_sort_candidates", "seg_nms", "seg_roi_align_f32", "seg_box_predict", "seg_finalize_detections",
                                                     "seg_point_sample_f32", "seg_upsample2x_f32", "seg_topk_points", "seg_point_logit_scatter", "seg_paste_masks"}
    for fn, text, args in sr.OPS_REFUSALS:
        a = [C.c_void_p(4096) if v is kit.PTR else v for v in args] + [None]
        assert getattr(hip_lib, fn)(*a) == -1, (fn, args)
        msg = hip_lib.coma_last_error().decode()
        assert msg.startswith(fn + ":") and re.search(text, msg), (fn, msg)
    one = C.c_void_p(4096)
    arr, dims = (C.c_void_p * 7)(*[4096] * 7), (C.c_int * 7)(*[4] * 7)
    assert hip_lib.seg_rpn_select_levels(arr, arr, dims, dims, 7, 4, 16, 1, 10, 64.0, 64.0, 8192, one, one, one, None, None) == -1
    assert b"1 .. 6 levels, got 7" in hip_lib.coma_last_error()
    assert hip_lib.seg_rpn_select_levels(arr, arr, dims, dims, 2, 4, 16, 1, 10, 64.0, 64.0, 19, one, one, one, None, None) == -1
    assert b"20 candidates exceed the list capacity 19" in hip_lib.coma_last_error()


def test_operator_tables_cover_the_branches():
    assert {n for n, _ in sr.MEMSET_CASES} == {1, 15, 16, 17, 4101} and {o for _, o in sr.MEMSET_CASES} == {0, 1, 8}
    assert {h for h, _, _ in sr.POOL_CASES} | {w for _, w, _ in sr.POOL_CASES} == {1, 2, 7, 8} and {c for _, _, c in sr.POOL_CASES} == {4, 68}
    assert bool(torch.isinf(sr.make_pool_input(7, 8, 68)).any())
    ks = [(so.bilinear_coeffs(h, nh)[1].shape[1], so.bilinear_coeffs(w, nw)[1].shape[1], h, nh, r) for _, h, w, nh, nw, _, _, r in sr.RESIZE_CASES]
    assert any(nh > h for _, _, h, nh, _ in ks) and any(max(a, b) > 3 for a, b, *_ in ks) and any(h == nh == 1 for _, _, h, nh, _ in ks) and any(not r for *_, r in ks)
    rp = {c.id: c for c in sr.RPN_CASES}
    six = rp["six-levels-topk48"]
    assert len(six.dims) == 6 and any(n < 48 for n in six.counts) and any(n == 48 for n in six.counts) and any(n > 48 for n in six.counts)
    assert rp["one-level-n-is-topk-plus-1"].counts == [48] and rp["one-level-n-is-topk-plus-1"].pre_topk == 47
    assert rp["one-level-9000-second-strip-round"].counts[0] > 8192 and all(c.batch == 3 for c in sr.RPN_CASES)
    for c in sr.RPN_CASES:                                     # ties do straddle the cut, +0 and -0 both occur, something is dropped after selection
        preds = sr.make_rpn_preds(c)
        lg = preds[0][0, :, :3].reshape(-1)
        if lg.numel() > c.pre_topk:
            kth = torch.sort(lg, descending=True)[0][c.pre_topk - 1]
            assert int((lg == kth).sum()) > int((lg[so.topk_stable(lg, c.pre_topk)] == kth).sum()) >= 2       # some of the equal logits are taken, some not
        z = torch.cat([p[..., :3].reshape(-1) for p in preds])
        assert bool(((z == 0) & torch.signbit(z)).any()) and bool(((z == 0) & ~torch.signbit(z)).any())
        assert any(int((~l["ok"]).sum()) for l in sr.rpn_reference(c, preds)[0])
    assert sr.SORT_CAPS == (64, 128, 1024, 8192) and {n for n, _ in sr.sort_variants(1024)} >= {0, 1, 63, 64, 65, 1024}
    assert {c.cap for c in sr.NMS_CASES} == {64, 128, 8192} and {n for c in sr.NMS_CASES for n in c.n} >= {0, 1, 64, 65, 4097}
    assert any(c.max_keep == 1 for c in sr.NMS_CASES) and any(c.max_keep > max(c.n) for c in sr.NMS_CASES)
    for c in sr.NMS_CASES:
        b = sr.make_nms_inputs(c)
        kept = [len(so.nms_ref(torch.from_numpy(b[0][i, :n]), torch.from_numpy(b[1][i, :n]), b[2][i, :n], c.thresh)) if n else 0 for i, n in enumerate(c.n)]
        if "mid-block" in c.id:
            assert kept[0] > c.max_keep and c.max_keep % 64                      # the list is cut inside a block of 64
    assert {c.out_size for c in sr.ROI_CASES} == {1, 2, 7, 14, 16} and {c.c for c in sr.ROI_CASES} == {4, 260}
    assert {(c.h2, c.w2) for c in sr.ROI_CASES} >= {(8, 8), (16, 24)} and any(0 in c.counts for c in sr.ROI_CASES)
    assert {c.ld for c in sr.BOXPRED_CASES} == {401, 404} and any(len(c.counts) * c.R % 4 for c in sr.BOXPRED_CASES) and any(0 in c.counts for c in sr.BOXPRED_CASES)
    assert {c.c for c in sr.SAMPLE_CASES} == {4, 80} and {c.P for c in sr.SAMPLE_CASES} == {1, 5, 196} and {c.n_copies for c in sr.SAMPLE_CASES} == {1, 3}
    assert any(len(c.counts) * c.R * c.P % 4 for c in sr.SAMPLE_CASES) and any(c.col0 and c.ldo > c.col0 + c.c for c in sr.SAMPLE_CASES)
    assert {(c.per_roi, c.grid) for c in sr.SAMPLE_CASES} == {(a, b) for a in (False, True) for b in (False, True)}
    assert sr.UPSAMPLE_SIDES == (1, 2, 7, 28) and sr.TOPK_CASES == [(1, 1), (7, 1), (7, 49), (28, 784), (70, 50)]
    assert {k for k, *_ in sr.LOGIT_CASES} == {3, 64, 336} and all(l > k for k, l, *_ in sr.LOGIT_CASES) and {i for *_, i in sr.LOGIT_CASES} == {True, False}
    assert {c.s for c in sr.PASTE_CASES} == {7, 28} and {c.R for c in sr.PASTE_CASES} == {1, 5} and any(not c.masks for c in sr.PASTE_CASES)
    assert any(c.cat_id for c in sr.PASTE_CASES) and all((c.out_h, c.out_w) == (16, 24) for c in sr.PASTE_CASES)


@pytest.mark.parametrize("case", sr.ROI_CASES, ids=lambda c: c.id)
def test_roi_reference_meets_its_bound(case):
    """The oracle's fp32 ROIAlign is within the bound of the float64 restatement (same fp32 sample geometry), levels are assign_levels'
    wherever the area is not negative, and the special boxes are what they are meant to be."""
    c = case
    feats, boxes = sr.make_roi_inputs(c)
    worst, kinds = 0.0, set()
    for b, n in enumerate(c.counts):
        bb = torch.from_numpy(boxes[b, :n])
        assert bool(torch.from_numpy(boxes[b, n:]).isnan().all())
        lv = sr.roi_levels_reference(bb)
        area = (bb[:, 2] - bb[:, 0]) * (bb[:, 3] - bb[:, 1])
        assert torch.equal(lv[area >= 0], so.assign_levels(bb[area >= 0]))
        for i in range(n):
            l = int(lv[i])
            ref, mag, samples = sr.roi_align_reference64(feats[l][b], boxes[b, i], c.out_size, 1.0 / (4 << l))
            w, h = float(bb[i, 2] - bb[i, 0]), float(bb[i, 3] - bb[i, 1])
            kinds.add("both-inverted" if w < 0 and h < 0 else "inverted" if min(w, h) < 0 else "empty" if min(w, h) == 0 else "plain")
            if samples == 0:
                assert float(ref.abs().max()) == 0.0 and min(w, h) <= 0
            if float(area[i]) > 0:
                o = so.roi_align_ref(feats[l][b], bb[i:i + 1], c.out_size, 1.0 / (4 << l))[0].double()
                if samples:
                    worst = max(worst, float(((o - ref).abs() / sr.roi_bound(samples, mag).clamp_min(1e-300)).max()))
                    assert max(-(-samples // 1), 1) <= 64 * 64 or c.kind in ("wide", "tall")
                else:
                    assert float(o.abs().max()) == 0.0
    print(f"SEG_DOMAIN roi_align {c.id}: oracle fp32 worst |err| / bound = {worst:.3f}")
    assert worst <= 1.0
    if c.kind == "mixed" and max(c.counts) >= 6:
        assert kinds == {"both-inverted", "inverted", "empty", "plain"}
    if c.kind == "levels":
        assert len(set(sr.roi_levels_reference(torch.from_numpy(boxes[0])).tolist())) == 4


def test_box_predictor_threshold_exclusion_cap():
    """At most 2 candidates per case within 1e-6 of score_thresh (outside the row built to sit AT it); that row's probabilities equal the
    threshold exactly and give no candidate; the overflow case has more candidates than slots."""
    for c in sr.BOXPRED_CASES:
        pred, props = sr.make_boxpred_inputs(c)
        near = 0
        for b, n in enumerate(c.counts):
            ref = sr.boxpred_reference(c, pred, props, b)
            near += len(sr.boxpred_border(c, ref, (0,) if b == 0 else ()))
            if b == 0:
                assert bool((ref["probs"][0] == np.float32(1.0) / np.float32(81.0)).all()) and not bool(torch.isfinite(ref["probs"][1]).any())
                assert not bool(((ref["cand_inds"][:, 0] == 0) | (ref["cand_inds"][:, 0] == 1)).any())
                if "exact" in c.id:
                    assert float(ref["probs"][0, 0]) == c.thresh
            if "overflow" in c.id and b == 0:
                assert len(ref["cand_inds"]) > c.cap
            assert bool(pred[b * c.R + n:(b + 1) * c.R].isnan().all()) and bool(pred[:, 401:].isnan().all())
        assert near <= 2, (c.id, near)


@pytest.mark.parametrize("case", sr.SAMPLE_CASES, ids=lambda c: c.id)
def test_point_sample_reference_is_the_oracles(case):
    """The float64 restatement (the kernel's fp32 coordinates) against point_sample / fine_features: the project's looser 1e-5."""
    c = case
    feat, boxes, coords = sr.make_sample_inputs(c)
    B = len(c.counts)
    cc = sr.sample_coords(c, coords, B * c.R)
    if coords is not None:
        assert {float(np.float32(v)) for v in sr.SPECIAL_COORDS[:4]} <= set(coords[~coords.isnan()].tolist()) or c.P == 1
    for b, n in enumerate(c.counts):
        for i in range(n):
            r = b * c.R + i
            ref, _ = sr.point_sample_reference64(c, feat[r if c.per_roi else b], None if boxes is None else boxes[b, i], cc[r])
            o = so.point_sample(feat[r:r + 1], cc[r:r + 1])[0].t() if c.per_roi else \
                so.fine_features(feat[b:b + 1], torch.from_numpy(boxes[b, i:i + 1]), cc[r:r + 1].clone())[0].t()
            assert float((o.double() - ref).abs().max() / (o.abs().max() + 1e-30)) <= 1e-5


@pytest.mark.parametrize("case", sr.PASTE_CASES, ids=lambda c: c.id)
def test_paste_exclusion_cap(case):
    """At most 1 % of a case's pixels have a float64 blended probability within 1e-5 of 0.5, and outside them the oracle's fp32 masks are the
    float64 decision: the reference alone passes the device test."""
    c = case
    logits, boxes, valid, classes = sr.make_paste_inputs(c)
    excluded = total = 0
    for b, n in enumerate(c.counts):
        ref, p64 = sr.paste_reference(c, logits, boxes, valid, b)
        ok = torch.from_numpy(valid[b, :n]).bool()[:, None, None]
        skip = sr.paste_excluded(p64) & ok
        excluded, total = excluded + int(skip.sum()), total + n * c.out_h * c.out_w
        assert torch.equal(ref[~skip], ((p64 >= 0.5) & ok)[~skip])
        if b == 0 and c.R > 1:
            assert valid[0, :3].tolist() == [1, 1, 0] and int(ref[1].sum()) <= 1
    assert excluded <= 0.01 * max(total, 1) and total > 0


@pytest.mark.parametrize("s,k", sr.TOPK_CASES)
def test_topk_maps_hold_the_ties_they_name(s, k):
    m = sr.make_topk_maps(s, k)
    n = s * s
    assert float(m[1].abs().min()) == float(m[1].abs().max()) and bool((m[3] == 0).all())
    if n > 1:
        assert bool((m[2].reshape(-1)[0:n - n % 2:2] == -m[2].reshape(-1)[1:n:2]).all()) and bool(torch.signbit(m[3]).any()) and bool((~torch.signbit(m[3])).any())
    if k < n:
        a = torch.sort(m[4].abs().reshape(-1))[0]
        assert float(a[k - 1]) == float(a[k])                                      # equal |logit| on both sides of the cut
    idx, coords = sr.topk_reference(m[0], k)
    assert len(idx) == k and bool((idx[1:] > idx[:-1]).all()) and coords.shape == (k, 2)
