"""coma_contact_accumulate_f32 (coma_amd/csrc/contact.hip) and the three occupancy entry points of coma_amd/csrc/occupancy.hip
(coma_occupancy_splat, coma_occupancy_reduce, coma_occupancy_fused) through the C ABI -- raw pointers into guarded buffers, not the
Python classes -- over the domain their argument checks accept.  The tables are tests/contact_ref.CASES and tests/occupancy_ref.CASES;
tests/test_coma_core_ref_host.py checks on the CPU that they reach every regime and that a broken kernel fails them.

Per case: (a) contact_ref.check -- cnt and den bit for bit, nom and the two histograms within max(4 e_emu, floor) of the reference (per
row and per normal bin), the denormal promise -- or occupancy_ref.check -- counts, row sums, normalised grid, raw grid and field of all
three routes equal to the dense f64 reference in every bit, NaN-ness compared for NaNs; (b) what the contract says is written holds no
sentinel and, where the case is finite, no NaN / Inf; (c) guards (the workspace's included), and with S = 0 every output, keep their
first bits; (d) a second launch from identical state gives the same bits.  Operands sit between NaN guards, the object rows a
shared-object launch must not read are NaN, and every operand comes back as it went in.  Two launches (per route) and one synchronize per
case; every case is inside the accepted domain."""
import ctypes

import numpy as np
import pytest
import torch

from tests import contact_ref as cr
from tests import domain_kit as kit
from tests import occupancy_ref as orf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = kit.GUARD
f32, f64 = np.float32, np.float64


def _upload(buf):
    return torch.from_numpy(np.ascontiguousarray(buf)).to(DEV)


def _ptr(t):
    return t.data_ptr() + G * t.element_size()


def _launch(lib, entry, kw, what):
    rc = kit.call(lib, entry, kw, None)
    if rc == kit.COMA_E_INVALID:
        pytest.fail(f"{what}: refused inside the accepted domain: {lib.coma_last_error().decode()}")
    if rc != 0:
        raise RuntimeError(f"{entry} returned {rc}: {lib.coma_last_error().decode()}")


def _written(name, first, second, start, owns, finite):
    """kit.check_written on host copies with their guards: `owns` says whether the launch writes the body at all"""
    may = torch.zeros(start.size, dtype=torch.bool)
    if owns:
        may[G:-G] = True
    kit.check_written(name, first, second, torch.from_numpy(start), may, may, finite=finite)


# ------------------------------------------------------------------------------------------------------------------ contact
@pytest.mark.parametrize("case", cr.CASES, ids=lambda c: c.id)
def test_contact_domain(hip_lib, case):
    c, d = case, cr.data(case.id)
    assert torch.cuda.is_available()
    S, H, O, N = c.S, c.H, c.O, c.N
    obj = lambda a: a if c.stride or S <= 1 else np.concatenate([a, np.full((S - 1,) + a.shape[1:], np.nan, f32)])   # rows a shared launch must not read
    host = dict(human_verts=d["hv"], human_normals=d["hn"], obj_verts=obj(d["ov"]), obj_normals=obj(d["on"]), sphere_grid=d["grid"])
    packed = {k: kit.pack_rows(v.reshape(1, -1) if v.size else np.zeros((1, 0), f32), np.nan) for k, v in host.items()}
    ins = {k: _upload(v) for k, v in packed.items()}
    names = dict(prob_h_wrt_o="P1", prob_o_wrt_h="P2", nom="nom", den="den", cnt="cnt")
    start = {k: kit.pack_rows(d["state"][v].reshape(1, -1), kit.sentinel(1, f32)[0]) for k, v in names.items()}
    pv, spv = (ctypes.c_float * 3)(*d["p"].tolist()), (ctypes.c_float * 3)(*d["sp"].tolist())

    def launch(bufs):
        kw = dict(obj_sample_stride=c.stride, S=S, H=H, O=O, N=N, principle_vec=ctypes.addressof(pv), sub_principle_vec=ctypes.addressof(spv),
                  spatial_grid_size=cr.SIZE, spatial_grid_thres=cr.THRES, normal_gaussian_sigma=c.sigma, eps=cr.EPS)
        kw.update({k: _ptr(t) for k, t in ins.items()})
        kw.update({k: _ptr(t) for k, t in bufs.items()})
        _launch(hip_lib, "coma_contact_accumulate_f32", kw, c.id)

    first, second = kit.launch_twice(lambda: {k: _upload(v) for k, v in start.items()}, launch, c.id)
    got = {}
    finite = not c.special
    for k, v in names.items():
        a, b = first[k].cpu(), second[k].cpu()
        _written(k, a, b, start[k], owns=S > 0, finite=finite)
        got[v] = a.numpy()[G:-G]
    for k, t in ins.items():                                       # operands come back as they went in
        assert np.array_equal(kit.bits(t.cpu().numpy()), kit.bits(packed[k])), f"operand `{k}` was written"
    fig = cr.check(c, got)                                          # (a)
    for k, f in fig.items():
        print(f"CONTACT_DOMAIN {c.id} out={k} e_emu={f.e_emu:.3e} bound={f.bound:.3e} device={f.err:.3e}")
    print(f"CONTACT_DOMAIN {c.id} out=cnt,den exact" + (" S=0: nothing written" if S == 0 else ""))


# ------------------------------------------------------------------------------------------------------------------ occupancy
@pytest.mark.parametrize("case", orf.CASES, ids=lambda c: c.id)
def test_occupancy_domain(hip_lib, case):
    c, d = case, orf.data(case.id)
    assert torch.cuda.is_available()
    S, H, R = d["S"], c.H, c.R
    R3 = R ** 3
    packed = dict(q=kit.pack_rows(d["q"].reshape(1, -1), np.nan), centers=kit.pack_rows(d["cen"].reshape(1, -1), np.nan))
    if d["select"] is not None:
        packed["select"] = kit.pack_rows(d["select"].reshape(1, -1), np.uint8(1))        # a guard byte read as a flag selects a row
    ins = {k: _upload(v) for k, v in packed.items()}
    sel = _ptr(ins["select"]) if "select" in ins else 0
    ws_bytes = orf.workspace_bytes(hip_lib, c)
    assert ws_bytes > 0 and ws_bytes % 16 == 0
    sent = lambda n: kit.sentinel(G + n + G, f32)
    zeros = kit.pack_rows(np.zeros((1, H * R3), f32), kit.sentinel(1, f32)[0])
    common = dict(q=_ptr(ins["q"]), S=S, H=H, R=R, centers=_ptr(ins["centers"]), voxel=d["voxel"], thres=d["thres"])

    def make():
        out = {}
        for route in orf.ROUTES:
            o = dict(counts=_upload(zeros if route == "splat" else sent(H * R3)), rowsum=_upload(sent(H)), out=_upload(sent(R3)))
            if route != "splat":
                o["workspace"] = _upload(sent(ws_bytes // 4))   # exactly the bytes the entry point asks for, between sentinel guards
            out[route] = o
        return out

    def launch(bufs):
        for route, o in bufs.items():
            if route == "splat":
                _launch(hip_lib, "coma_occupancy_splat", dict(common, counts=_ptr(o["counts"])), c.id)
                o["raw"] = o["counts"].clone()
                if not c.big:
                    _launch(hip_lib, "coma_occupancy_reduce", dict(counts=_ptr(o["counts"]), select=sel, H=H, R3=R3, rowsum=_ptr(o["rowsum"]), out=_ptr(o["out"])), c.id)
            else:
                _launch(hip_lib, "coma_occupancy_fused", dict(common, thres_sq_cut=d["t2"], window=d["window"], select=sel, write_raw=int(route == "fused_raw"),
                                                              counts=_ptr(o["counts"]), rowsum=_ptr(o["rowsum"]), out=_ptr(o["out"]), workspace=_ptr(o["workspace"]),
                                                              workspace_bytes=ws_bytes), c.id)

    first, second = kit.launch_twice(make, launch, c.id)
    got = {}
    for route in orf.ROUTES:
        got[route] = {}
        for k in ("counts", "rowsum", "out", "raw"):
            if k not in first[route]:
                continue
            a, b = first[route][k].cpu(), second[route][k].cpu()
            owns = not (c.big and route == "splat" and k in ("rowsum", "out"))       # (above 2^24 the reducer is not run)
            _written(f"{route}.{k}", a, b, (zeros if k == "raw" else sent(a.numel() - 2 * G)), owns=owns, finite=False)
            got[route][k] = a.numpy()[G:-G]
        if "workspace" in first[route]:                             # (c) for the workspace; its contents depend on the order of the atomics
            for w in (first[route]["workspace"], second[route]["workspace"]):
                w = w.cpu().numpy()
                assert bool((kit.bits(w[:G]) == kit.sentinel_bits(f32)).all() and (kit.bits(w[-G:]) == kit.sentinel_bits(f32)).all()), f"(c) {route}: a guard of the workspace was written"
    for k, t in ins.items():
        assert np.array_equal(kit.bits(t.cpu().numpy()), kit.bits(packed[k])), f"operand `{k}` was written"
    n = orf.check(c, got)                                           # (a)
    print(f"OCC_DOMAIN {c.id} routes={','.join(orf.compared_routes(c))} elements={n} exact")


@pytest.mark.parametrize("cid", ["occ-r8-w4", "occ-r30-w7"])
def test_reduce_takes_the_one_cell_kernels_when_misaligned(hip_lib, cid):
    """R3 % 4 == 0 with `counts` and `out` 4 bytes off a 16-byte boundary: coma_occupancy_reduce accepts them and gives the same bits
    (the splat has no 16-byte access).  The buffers are guard | one poison element | data | guard."""
    c, d, ref = orf.BY_ID[cid], orf.data(cid), orf.reference(cid)
    assert torch.cuda.is_available() and c.R ** 3 % 4 == 0
    S, H, R3 = d["S"], c.H, c.R ** 3
    sv = kit.sentinel(1, f32)[0]
    ins = dict(q=_upload(kit.pack_rows(d["q"].reshape(1, -1), np.nan)), centers=_upload(kit.pack_rows(d["cen"].reshape(1, -1), np.nan)))
    sel = 0
    if d["select"] is not None:
        ins["select"] = _upload(kit.pack_rows(d["select"].reshape(1, -1), np.uint8(1)))
        sel = _ptr(ins["select"])
    start = dict(counts=kit.pack_rows(np.zeros((1, H * R3), f32), sv, off=1), rowsum=kit.pack_rows(np.full((1, H), sv, f32), sv),
                 out=kit.pack_rows(np.full((1, R3), sv, f32), sv, off=1))
    off = dict(counts=4, rowsum=0, out=4)

    def launch(bufs):
        p = {k: _ptr(t) + off[k] for k, t in bufs.items()}
        assert p["counts"] % 16 == 4 and p["out"] % 16 == 4
        _launch(hip_lib, "coma_occupancy_splat", dict(q=_ptr(ins["q"]), S=S, H=H, R=c.R, centers=_ptr(ins["centers"]), voxel=d["voxel"], thres=d["thres"],
                                                      counts=p["counts"]), cid)
        _launch(hip_lib, "coma_occupancy_reduce", dict(counts=p["counts"], select=sel, H=H, R3=R3, rowsum=p["rowsum"], out=p["out"]), cid)

    first, second = kit.launch_twice(lambda: {k: _upload(v) for k, v in start.items()}, launch, cid)
    got = {}
    for k, v in start.items():
        a, b = first[k].cpu(), second[k].cpu()
        may = torch.zeros(v.size, dtype=torch.bool)
        may[G + off[k] // 4:-G] = True
        kit.check_written(k, a, b, torch.from_numpy(v), may, may, finite=False)
        got[k] = a.numpy()[G + off[k] // 4:-G]
    orf.same(got["rowsum"], ref["rowsum"], f"{cid} rowsum")
    orf.same(got["counts"].reshape(H, R3), ref["norm"], f"{cid} counts")
    orf.same(got["out"], ref["field"], f"{cid} out")


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_reported_not_launched(hip_lib):
    """Every row of contact_ref.REFUSALS and occupancy_ref.REFUSALS through the real entry points, with small device buffers where the row
    wants a pointer -- the misaligned rows included: none of them is launched, and every output buffer keeps its sentinel."""
    assert torch.cuda.is_available()
    refusals = {**cr.REFUSALS, **orf.REFUSALS}
    resolve, outs, small = kit.device_resolver(cr.OUTPUT_ARGS + orf.OUTPUT_ARGS, cr.HOST_ARGS)
    assert kit.check_refusals(hip_lib, refusals, resolve, expect_control=False) >= 80
    kit.refusal_outputs_untouched(outs, small)
