"""The rasteriser (coma_raster_depth_f64, coma_silhouette_iou), the volume and column kernels (coma_mesh_volume_f64,
coma_intersection_columns) and the shift profile and depth optimiser (coma_shift_columns_prepare, coma_shift_profile,
coma_depth_optimize_f64) with their status functions, through the C ABI -- raw pointers into guarded buffers, not the Python wrappers --
over the domain their argument checks accept.  The tables are tests/column_ref.CASES, DEVICE_REFUSALS and REFUSALS;
tests/test_column_ref_host.py checks on the CPU that they reach every regime and that a broken kernel fails them.

Per case: (a) column_ref.check -- keys, counts, masks, sums, per-column maps, lengths, profiles, trajectories and the status / epoch
equal to the restatements in every bit, the volume equal to mesh_volume_shape in every bit, the work lists as long as the emulation
says; (b) what the contract says is written holds no sentinel; (c) guards, the workspaces' included, and every output or slot the
contract leaves alone keep their first bits, and operands come back as they went in; (d) a second launch gives the same bits.
Operands sit between NaN guards (face tables and cand_view between zeros: a guard can never send a kernel outside a buffer), every
workspace is exactly as long as its size function says, between guards.  Two launches and one synchronize per case; every case is
inside the accepted domain or refused by a check the kernels make before they follow the data."""
import ctypes

import numpy as np
import pytest
import torch

from tests import column_ref as cr
from tests import domain_kit as kit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = kit.GUARD
WG = 4096                                    # guard bytes on either side of a workspace (keeps its 16-byte alignment)
f64, i32, i64, u8, u64 = np.float64, np.int32, np.int64, np.uint8, np.uint64
IDS = lambda c: c.id


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return 0 if t is None else t.data_ptr() + G * t.element_size()


def _wptr(t):
    return t.data_ptr() + WG


class Ins:
    """operands between guards: NaN for floats, 0 for index tables, the sentinel for everything else; checked on the way out"""

    def __init__(self, **arrays):
        self.host, self.dev = {}, {}
        for k, a in arrays.items():
            if a is None or a.size == 0:
                self.dev[k] = None
                continue
            poison = np.nan if a.dtype.kind == "f" else 0 if a.dtype == i32 else kit.sentinel(1, a.dtype)[0]
            self.host[k] = kit.pack_rows(a.reshape(1, -1), poison)
            self.dev[k] = _up(self.host[k])

    def ptr(self, k):
        return _ptr(self.dev[k])

    def unchanged(self):
        for k, h in self.host.items():
            assert np.array_equal(kit.bits(self.dev[k].cpu().numpy()), kit.bits(h)), f"operand `{k}` was written"


def _sent(n, dtype):
    return _up(kit.sentinel(G + n + G, dtype))


def _workspace(nbytes):
    assert nbytes > 0
    return _up(kit.sentinel(WG + nbytes + WG, u8))


def _workspace_guards(name, *bufs, nbytes):
    for w in bufs:
        w = w.cpu().numpy()
        assert w.size == 2 * WG + nbytes and (w[:WG] == 0xA5).all() and (w[-WG:] == 0xA5).all(), f"(c) a guard of the workspace `{name}` was written"


def _header(ws, skip=0):
    """the 16 ints of a columns / raster workspace header"""
    return ws.cpu().numpy()[WG + skip:WG + skip + 64].view(i32)


def _ok(lib, rc, what):
    if rc == kit.COMA_E_INVALID:
        pytest.fail(f"{what}: refused inside the accepted domain: {lib.coma_last_error().decode()}")
    if rc != 0:
        raise RuntimeError(f"{what} returned {rc}: {lib.coma_last_error().decode()}")


def _call(lib, entry, kw, what):
    _ok(lib, kit.call(lib, entry, kw, None), f"{what} {entry}")


def _written(name, first, second, n_may, n_must=None, start=None):
    """kit.check_written on an output with guards: the first n_may elements of the body may, the first n_must must be written"""
    a, b = first.cpu(), second.cpu()
    may = torch.zeros(a.numel(), dtype=torch.bool)
    may[G:G + n_may] = True
    must = may.clone()
    if n_must is not None:
        must[:] = False
        must[G:G + n_must] = True
    start = torch.from_numpy(kit.sentinel(a.numel(), a.numpy().dtype)) if start is None else start
    kit.check_written(name, a, b, start, must, may, finite=False)
    return a.numpy()[G:-G]


def _doubles(*v):
    return (ctypes.c_double * len(v))(*[float(x) for x in v])


# ------------------------------------------------------------------------------------------------------------------ rasteriser
def _raster_kw(ins, d, V, F, W, H, R, t):
    return dict(verts=ins.ptr("verts"), V=V, faces=ins.ptr("faces"), F=F, R=ctypes.addressof(R), t=ctypes.addressof(t), scale=float(d["scale"]), W=W, H=H)


@pytest.mark.parametrize("case", cr.KIND("raster"), ids=IDS)
def test_raster_domain(hip_lib, case):
    c, d = case, cr.data(case.id)
    V, F, n = len(d["verts"]), len(d["faces"]), c.W * c.H
    ins = Ins(verts=d["verts"].astype(f64), faces=d["faces"].astype(i32))
    R, t = _doubles(*np.asarray(d["R"]).reshape(-1)), _doubles(*np.asarray(d["t"]).reshape(-1))
    nbytes = int(hip_lib.coma_raster_workspace_bytes(V, F))
    base = _raster_kw(ins, d, V, F, c.W, c.H, R, t)
    make = lambda: dict(depth_key=_sent(n, i64), workspace=_workspace(nbytes))
    launch = lambda o: _call(hip_lib, "coma_raster_depth_f64", dict(base, workspace=_wptr(o["workspace"]), depth_key=_ptr(o["depth_key"])), c.id)
    first, second = kit.launch_twice(make, launch, c.id)
    for o in (first, second):
        _ok(hip_lib, hip_lib.coma_raster_status(_wptr(o["workspace"]), None), f"{c.id} coma_raster_status")
    key = _written("depth_key", first["depth_key"], second["depth_key"], n)
    _workspace_guards("workspace", first["workspace"], second["workspace"], nbytes=nbytes)
    ins.unchanged()
    hdr = _header(first["workspace"])
    compared = cr.check(c, dict(key=key.view(u64).reshape(c.H, c.W), stat=dict(listed=int(hdr[1]))))
    if "raster-hits-full" in cr.branches(c.id):                    # from the list in the device's own order of arrival: a step with hits[] full
        for o in (first, second):
            big = o["workspace"].cpu().numpy()[WG + 64 + 16 * V:WG + nbytes].view(i32)
            assert cr.tile_0_hits(big, int(hdr[1]))[0] == 256, f"{c.id}: no step of the work list fills hits[] on tile 0"
    print(f"COLUMN_DOMAIN {c.id} keys={compared} listed={int(hdr[1])} workspace={nbytes} exact")


@pytest.mark.parametrize("case", cr.KIND("iou"), ids=IDS)
def test_silhouette_domain(hip_lib, case):
    c, d = case, cr.data(case.id)
    n, K = c.W * c.H, c.K
    ins = Ins(human_key=d["human"].view(i64), asset_key=None if d["asset"] is None else d["asset"].view(i64), offsets=d["offsets"], gt=d["gt"])
    base = dict(human_key=ins.ptr("human_key"), asset_key=ins.ptr("asset_key"), offsets=ins.ptr("offsets"), K=K, gt=ins.ptr("gt"), W=c.W, H=c.H)

    def make():
        o = {k: _sent(64, i64) for k in ("visible", "inter", "uni")}
        o["masks"] = _sent(K * n, u8) if c.masks else None
        return o
    launch = lambda o: _call(hip_lib, "coma_silhouette_iou", dict(base, **{k: _ptr(v) for k, v in o.items()}), c.id)
    first, second = kit.launch_twice(make, launch, c.id)
    got = {k: _written(k, first[k], second[k], K)[:K] for k in ("visible", "inter", "uni")}           # the slots [K, 64) keep their sentinel
    got["masks"] = _written("masks", first["masks"], second["masks"], K * n).reshape(K, c.H, c.W) if c.masks else None
    ins.unchanged()
    print(f"COLUMN_DOMAIN {c.id} compared={cr.check(c, got)} visible={got['visible'][:3].tolist()} exact")


# ------------------------------------------------------------------------------------------------------------------ volume
@pytest.mark.parametrize("case", cr.KIND("volume"), ids=IDS)
def test_mesh_volume_domain(hip_lib, case):
    c, d = case, cr.data(case.id)
    V, F = len(d["verts"]), len(d["faces"])
    ins = Ins(verts=d["verts"].astype(f64), faces=d["faces"].astype(i32))
    nbytes = int(hip_lib.coma_mesh_volume_workspace_bytes(F))
    assert nbytes == 8 * min(-(-F // 256), 256)
    make = lambda: dict(out=_sent(1, f64), workspace=_workspace(nbytes))
    launch = lambda o: _call(hip_lib, "coma_mesh_volume_f64", dict(verts=ins.ptr("verts"), V=V, faces=ins.ptr("faces"), F=F, out=_ptr(o["out"]), workspace=_wptr(o["workspace"])), c.id)
    first, second = kit.launch_twice(make, launch, c.id)
    out = _written("out", first["out"], second["out"], 1)
    _workspace_guards("workspace", first["workspace"], second["workspace"], nbytes=nbytes)
    assert np.array_equal(first["workspace"].cpu().numpy(), second["workspace"].cpu().numpy()), "(d) the partial sums differ"
    ins.unchanged()
    cr.check(c, dict(out=float(out[0])))
    print(f"COLUMN_DOMAIN {c.id} F={F} volume={float(out[0])!r} equal to the summation shape in every bit")


# ------------------------------------------------------------------------------------------------------------------ columns, profile
def _meshes(d):
    return Ins(vertsA=d["A"][0].astype(f64), facesA=d["A"][1].astype(i32), vertsB=d["B"][0].astype(f64), facesB=d["B"][1].astype(i32))


def _columns_kw(ins, d, W, H, capacity):
    return dict(vertsA=ins.ptr("vertsA"), VA=len(d["A"][0]), facesA=ins.ptr("facesA"), FA=len(d["A"][1]), vertsB=ins.ptr("vertsB"), VB=len(d["B"][0]),
                facesB=ins.ptr("facesB"), FB=len(d["B"][1]), x0=d["x0"], y0=d["y0"], s=d["s"], W=W, H=H, capacity=capacity)


def _sizes(kw):
    return tuple(kw[k] for k in ("VA", "FA", "VB", "FB", "W", "H", "capacity"))


def _status(lib, entry, ws):
    needed = ctypes.c_int64(-1)
    rc = getattr(lib, entry)(_wptr(ws), None, ctypes.byref(needed))
    return rc, lib.coma_last_error().decode() if rc else "", needed.value


@pytest.mark.parametrize("case", cr.KIND("columns"), ids=IDS)
def test_columns_and_profile_domain(hip_lib, case):
    c, d, ref = case, cr.data(case.id), cr.reference(case.id)
    n, batches = c.W * c.H, cr.shifts(case.id)
    ins = _meshes(d)
    dins = Ins(**{f"d{k}": b for k, b in enumerate(batches)})
    kw = _columns_kw(ins, d, c.W, c.H, max(ref["needed"], 1))         # capacity equal to the count
    b1, b2 = int(hip_lib.coma_column_crossings_workspace_bytes(*_sizes(kw))), int(hip_lib.coma_shift_columns_workspace_bytes(*_sizes(kw)))

    def make():
        o = dict(sums=_sent(3, i64), col_ab=_sent(n, i64) if c.col_ab else None, ws1=_workspace(b1), lengths=_sent(2, i64) if c.lengths else None, ws2=_workspace(b2))
        o.update({f"L{k}": _sent(3 * len(b), i64) for k, b in enumerate(batches)})
        return o

    def launch(o):
        _call(hip_lib, "coma_intersection_columns", dict(kw, workspace=_wptr(o["ws1"]), sums=_ptr(o["sums"]), col_ab=_ptr(o["col_ab"])), c.id)
        _call(hip_lib, "coma_shift_columns_prepare", dict(kw, workspace=_wptr(o["ws2"]), lengths=_ptr(o["lengths"])), c.id)
        for k, b in enumerate(batches):
            _call(hip_lib, "coma_shift_profile", dict(workspace=_wptr(o["ws2"]), d=dins.ptr(f"d{k}"), K=len(b), L=_ptr(o[f"L{k}"])), c.id)
    first, second = kit.launch_twice(make, launch, c.id)
    needed = set()
    for o in (first, second):
        for entry, ws in (("coma_intersection_status", o["ws1"]), ("coma_shift_columns_status", o["ws2"])):
            rc, text, need = _status(hip_lib, entry, ws)
            _ok(hip_lib, rc, f"{c.id} {entry}")
            needed.add(need)
    assert len(needed) == 1
    got = dict(sums=_written("sums", first["sums"], second["sums"], 3), needed=needed.pop(),
               col_ab=_written("col_ab", first["col_ab"], second["col_ab"], n).reshape(c.H, c.W) if c.col_ab else None,
               lengths=_written("lengths", first["lengths"], second["lengths"], 2) if c.lengths else None,
               L=[_written(f"L{k}", first[f"L{k}"], second[f"L{k}"], 3 * len(b)).reshape(len(b), 3) for k, b in enumerate(batches)])
    _workspace_guards("intersection workspace", first["ws1"], second["ws1"], nbytes=b1)
    _workspace_guards("shift workspace", first["ws2"], second["ws2"], nbytes=b2)
    ins.unchanged(), dins.unchanged()
    h1, h2 = _header(first["ws1"]), _header(first["ws2"], skip=64)
    assert (int(h1[1]), int(h1[2])) == (int(h2[1]), int(h2[2]))
    got["stat"] = dict(A=dict(listed=int(h1[1])), B=dict(listed=int(h1[2])))
    compared = cr.check(c, got)
    print(f"COLUMN_DOMAIN {c.id} crossings={got['needed']} longest column={int(ref['counts'].max())} listed={int(h1[1])}+{int(h1[2])} launches of the profile={len(batches)} "
          f"compared={compared} workspaces={b1}+{b2} exact")


# ------------------------------------------------------------------------------------------------------------------ optimiser
@pytest.fixture(scope="module")
def prepared(hip_lib):
    """a prepared shift workspace per column case, exactly sized between guards, made once: coma_depth_optimize_f64 only reads it"""
    cache = {}

    def get(cid):
        if cid in cache:
            return cache[cid]
        c, d = cr.BY_ID[cid], cr.data(cid)
        ins = _meshes(d)
        kw = _columns_kw(ins, d, c.W, c.H, max(cr.reference(cid)["needed"], 1))
        nbytes = int(hip_lib.coma_shift_columns_workspace_bytes(*_sizes(kw)))
        ws = _workspace(nbytes)
        with kit.device_guard(f"prepare {cid}"):
            _call(hip_lib, "coma_shift_columns_prepare", dict(kw, workspace=_wptr(ws), lengths=0), cid)
        _ok(hip_lib, _status(hip_lib, "coma_shift_columns_status", ws)[0], f"prepare {cid}")
        cache[cid] = (ws, nbytes)
        return ws, nbytes
    return get


OPT_TEXT = {"cand_view holds an index": 3, "holds a refused call": 2, "d is not finite": 1}


def _optimize_status(lib, state):
    epoch = ctypes.c_int(-1)
    rc = lib.coma_depth_optimize_status(_ptr(state), None, ctypes.byref(epoch))
    if rc == 0:
        return 0, 0, ""
    text = lib.coma_last_error().decode()
    assert rc == kit.COMA_E_INVALID, (rc, text)
    return [v for k, v in OPT_TEXT.items() if k in text][0], epoch.value, text


def _optimize_outputs(E):
    return dict(traj=_sent(E + 1, f64), Ltraj=_sent(3 * E, i64), losses=_sent(2 * E, f64), state=_sent(8, i64))


@pytest.mark.parametrize("case", cr.KIND("optimize"), ids=IDS)
def test_depth_optimize_domain(hip_lib, prepared, case):
    c, d = case, cr.data(case.id)
    assert int(hip_lib.coma_depth_optimize_state_bytes()) == 64
    ws, nbytes = prepared(c.columns) if c.ws else (None, 0)
    ws0 = ws.cpu().numpy().copy() if c.ws else None
    ins = Ins(views=d["views"], joints0=d["joints0"], cand_view=d["cand_view"], cand_xy=d["cand_xy"])
    front = _doubles(*d["front"])
    kw = dict(workspace=_wptr(ws) if c.ws else 0, views=ins.ptr("views"), n_views=c.n_views, joints0=ins.ptr("joints0") if c.N else 0, front=ctypes.addressof(front),
              cand_view=ins.ptr("cand_view"), cand_xy=ins.ptr("cand_xy"), N=c.N, J=c.J, d0=c.d0, lr=c.lr, w_multiview=c.w_mv, w_collision=c.w_col, E=c.E)
    launch = lambda o: _call(hip_lib, "coma_depth_optimize_f64", dict(kw, **{k: _ptr(v) for k, v in o.items()}), c.id)
    first, second = kit.launch_twice(lambda: _optimize_outputs(c.E), launch, c.id)
    status = [_optimize_status(hip_lib, o["state"]) for o in (first, second)]
    assert status[0] == status[1]
    w = cr.written(c)
    got = dict(status=status[0][0], epoch=status[0][1])
    for k, shape in (("traj", (c.E + 1,)), ("Ltraj", (c.E, 3)), ("losses", (c.E, 2))):
        got[k] = _written(k, first[k], second[k], w[k]).reshape(shape)     # (b) up to the stopping epoch, (c) the sentinel behind it
    _written("state", first["state"], second["state"], 8, n_must=6)
    ins.unchanged()
    if c.ws:
        assert np.array_equal(ws.cpu().numpy(), ws0), "the prepared workspace was written"
    compared = cr.check(c, got)
    print(f"COLUMN_DOMAIN {c.id} status={status[0][0]} epoch={status[0][1]} d={got['traj'][w['traj'] - 1]!r} written traj/Ltraj/losses={w['traj']}/{w['Ltraj']}/{w['losses']} "
          f"compared={compared} exact {status[0][2]}")


# ------------------------------------------------------------------------------------------------------------------ refusals on the device
def _untouched(name, *bufs):
    for t in bufs:
        a = t.cpu().numpy()
        assert (kit.bits(a) == kit.sentinel_bits(a.dtype)).all(), f"`{name}` was written by a refused call"


@pytest.mark.parametrize("mesh", [0, 1], ids=["meshA", "meshB"])
@pytest.mark.parametrize("row", cr.DEVICE_REFUSALS, ids=lambda r: r[0])
def test_device_side_refusals(hip_lib, prepared, row, mesh):
    kind, text, _, entries = row
    d = cr.refusal_data(kind, mesh)
    W = H = 32
    ins = _meshes(d)
    count = cr.reference(cr.REFUSAL_BASE)["needed"]
    want_needed = count if kind == "capacity" else 0              # 0 when the call was refused before the crossings were counted
    what = f"{kind} mesh {'AB'[mesh]}"
    if "raster" in entries:
        v, f = ("vertsA", "facesA") if mesh == 0 else ("vertsB", "facesB")
        R, t = _doubles(*cr.IDENT[0].reshape(-1)), _doubles(*cr.IDENT[1])
        V, F = len((d["A"], d["B"])[mesh][0]), len((d["A"], d["B"])[mesh][1])
        nbytes = int(hip_lib.coma_raster_workspace_bytes(V, F))
        kw = dict(verts=ins.ptr(v), V=V, faces=ins.ptr(f), F=F, R=ctypes.addressof(R), t=ctypes.addressof(t), scale=d["scale"], W=W, H=H)
        make = lambda: dict(depth_key=_sent(W * H, i64), workspace=_workspace(nbytes))
        launch = lambda o: _call(hip_lib, "coma_raster_depth_f64", dict(kw, workspace=_wptr(o["workspace"]), depth_key=_ptr(o["depth_key"])), what)
        first, second = kit.launch_twice(make, launch, what)
        for o in (first, second):
            rc = hip_lib.coma_raster_status(_wptr(o["workspace"]), None)
            msg = hip_lib.coma_last_error().decode()
            assert rc == kit.COMA_E_INVALID and f"coma_raster_depth_f64: {text}" in msg and "depth map untouched)" in msg, (what, rc, msg)
            _untouched("depth_key", o["depth_key"])
            _workspace_guards("workspace", o["workspace"], nbytes=nbytes)
    if "columns" not in entries:
        ins.unchanged()
        return
    kw = _columns_kw(ins, d, W, H, d["capacity"])
    b1, b2 = int(hip_lib.coma_column_crossings_workspace_bytes(*_sizes(kw))), int(hip_lib.coma_shift_columns_workspace_bytes(*_sizes(kw)))
    dd = Ins(d=np.array([0.0, 0.5], f64))
    front = _doubles(0.0, 0.0, 1.0)

    def make():
        return dict(sums=_sent(3, i64), col_ab=_sent(W * H, i64), ws1=_workspace(b1), lengths=_sent(2, i64), ws2=_workspace(b2), L=_sent(6, i64), **_optimize_outputs(3))

    def launch(o):
        _call(hip_lib, "coma_intersection_columns", dict(kw, workspace=_wptr(o["ws1"]), sums=_ptr(o["sums"]), col_ab=_ptr(o["col_ab"])), what)
        _call(hip_lib, "coma_shift_columns_prepare", dict(kw, workspace=_wptr(o["ws2"]), lengths=_ptr(o["lengths"])), what)
        _call(hip_lib, "coma_shift_profile", dict(workspace=_wptr(o["ws2"]), d=dd.ptr("d"), K=2, L=_ptr(o["L"])), what)      # against the refused workspace: L untouched
        _call(hip_lib, "coma_depth_optimize_f64", dict(workspace=_wptr(o["ws2"]), views=0, n_views=0, joints0=0, front=ctypes.addressof(front), cand_view=0, cand_xy=0, N=0,
                                                         J=25, d0=0.0, lr=0.01, w_multiview=0.0, w_collision=0.4, E=3, traj=_ptr(o["traj"]), Ltraj=_ptr(o["Ltraj"]),
                                                         losses=_ptr(o["losses"]), state=_ptr(o["state"])), what)
    first, second = kit.launch_twice(make, launch, what)
    for o in (first, second):
        for entry, ws, of, tail in (("coma_intersection_status", o["ws1"], "coma_intersection_columns", "sums untouched)"),
                                    ("coma_shift_columns_status", o["ws2"], "coma_shift_columns_prepare", "nothing written)")):
            rc, msg, need = _status(hip_lib, entry, ws)
            assert rc == kit.COMA_E_INVALID and f"{of}: {text}" in msg and tail in msg and need == want_needed, (what, entry, rc, msg, need)
            if kind == "capacity":
                assert f"{count} crossings needed" in msg
        assert _optimize_status(hip_lib, o["state"])[0] == 2
        for k in ("sums", "col_ab", "lengths", "L", "traj", "Ltraj", "losses"):
            _untouched(k, o[k])
        _workspace_guards("intersection workspace", o["ws1"], nbytes=b1)
        _workspace_guards("shift workspace", o["ws2"], nbytes=b2)
    ins.unchanged(), dd.unchanged()


# ------------------------------------------------------------------------------------------------------------------ argument checks
def test_refusals_are_reported_not_launched(hip_lib):
    """Every row of column_ref.REFUSALS through the real entry points, with small device buffers where the row wants a pointer -- the
    misaligned rows included: none of them is launched, and every output buffer keeps its sentinel."""
    assert torch.cuda.is_available()
    base, outs, small = kit.device_resolver(cr.OUTPUT_ARGS)
    resolve = cr.with_host_arrays(base)
    n = kit.check_refusals(hip_lib, cr.REFUSALS, resolve, expect_control=False) + cr.run_plain_refusals(hip_lib, resolve)
    covered, sites = cr.argument_check_sites()
    assert covered == sites and n >= 150
    kit.refusal_outputs_untouched(outs, small)
