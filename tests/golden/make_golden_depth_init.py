#!/usr/bin/env python3
"""Golden vectors for depth initialisation, produced by the REAL reference module
(/root/reference/src/generation/initialize_depth.py) with Blender stubbed out.

The reference's `initialize_depth()` is run end to end on a synthetic tree (inpaintings, camera pickles, human-prediction
pickles).  blenderproc, bpy, mathutils, trimesh, cv2 and tqdm are stand-ins: the scene functions keep a list of meshes,
`cv2.bitwise_and / bitwise_or / countNonZero` are NumPy, and `bproc.renderer.render_segmap` returns the instance map that
tests/raster_ref.py draws of the current scene (asset first, so the asset wins exact ties) -- Blender's own render is NOT
available and stays unpinned.  Everything else is the reference's own code: the pixel -> world transform, the asset transform,
compute_directional_size, compute_nearest_point, the displacement list, extract_candidates, select_human and the pickles it
writes.  Its functions are wrapped so that their arguments and results are recorded on the way.

Writes tests/golden/depth_init_golden.npz.   Run (build container only): python tests/golden/make_golden_depth_init.py
"""
import contextlib
import importlib
import io
import os
import pickle
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
RES = 64


class Scene:
    """What the stand-ins know of the Blender scene: the asset in world space and the meshes linked since."""
    def __init__(self):
        self.reset()
        self.renders = []                  # per render_segmap call: visible pixel count of the mesh rendered last

    def reset(self):
        self.asset, self.meshes, self.camera = None, [], None


SCENE = Scene()
COUNTS = []                                # cv2.countNonZero results in call order: (intersection, union) per visible candidate


def install_stubs():
    from tests import raster_ref as RR

    class _Any(types.ModuleType):
        def __getattr__(self, k):
            if k.startswith("__"):
                raise AttributeError(k)
            return lambda *a, **kw: None

    class Mesh:
        def __init__(self, name):
            self.name, self.verts, self.faces = name, None, None

        def from_pydata(self, verts, edges, faces):
            self.verts, self.faces = np.array(verts, dtype=np.float64), np.array(faces, dtype=np.int32)

        def update(self):
            pass

    class Objects(dict):
        def new(self, name, mesh):
            unique, n = name, 0
            while unique in self:          # Blender's SMPL, SMPL.001, ...
                n += 1
                unique = f"{name}.{n:03d}"
            obj = types.SimpleNamespace(name=unique, mesh=mesh)
            self[unique] = obj
            return obj

        def remove(self, obj, do_unlink=True):
            del self[obj.name]
            SCENE.meshes = [m for m in SCENE.meshes if m.name != obj.name]

    objects = Objects()
    collection = types.SimpleNamespace(objects=types.SimpleNamespace(link=lambda obj: SCENE.meshes.append(obj)))
    bpy = _Any("bpy")
    bpy.data = types.SimpleNamespace(collections=types.SimpleNamespace(new=lambda name: collection),
                                     meshes=types.SimpleNamespace(new=lambda name: Mesh(name)), objects=objects)
    bpy.context = types.SimpleNamespace(scene=types.SimpleNamespace(collection=types.SimpleNamespace(children=types.SimpleNamespace(link=lambda c: None))))
    handlers = _Any("bpy.app.handlers")
    handlers.persistent = lambda f: f
    app = _Any("bpy.app")
    app.handlers = handlers
    bpy.app = app

    def render_segmap(map_by=None):
        cam = SCENE.camera
        W, H = cam["resolution"]
        meshes = [SCENE.asset] + [(o.mesh.verts, o.mesh.faces) for o in SCENE.meshes]
        seg = RR.segmap(meshes, cam["R"], cam["t"], cam["scale"], W, H)
        names = ["asset"] + [o.name for o in SCENE.meshes]
        SCENE.renders.append(int((seg == len(meshes)).sum()))
        # blenderproc lists the instances that occur in the image
        return dict(instance_segmaps=[seg], instance_attribute_maps=[[dict(idx=i + 1, name=n) for i, n in enumerate(names) if (seg == i + 1).any()]])

    bproc = _Any("blenderproc")
    bproc.renderer = types.SimpleNamespace(render_segmap=render_segmap)
    bproc.camera = types.SimpleNamespace(add_camera_pose=lambda m: None)
    bproc.utility = types.SimpleNamespace(reset_keyframes=lambda: None)

    cv2 = _Any("cv2")
    cv2.bitwise_and = lambda a, b: np.bitwise_and(a, b)
    cv2.bitwise_or = lambda a, b: np.bitwise_or(a, b)

    def count_non_zero(a):
        n = int(np.count_nonzero(a))
        COUNTS.append(n)
        return n
    cv2.countNonZero = count_non_zero

    mathutils = _Any("mathutils")
    mathutils.Matrix = lambda m: types.SimpleNamespace(to_euler=lambda order: None)
    tqdm = _Any("tqdm")

    class _Bar(list):
        def set_description(self, desc=None):
            pass
    tqdm.tqdm = lambda it, *a, **kw: _Bar(it)
    trimesh = _Any("trimesh")
    boolean = _Any("trimesh.boolean")
    boolean.intersection = lambda *a, **kw: None
    trimesh.boolean = boolean
    for name, mod in {"bpy": bpy, "bpy.app": app, "bpy.app.handlers": handlers, "blenderproc": bproc, "cv2": cv2, "mathutils": mathutils,
                      "tqdm": tqdm, "trimesh": trimesh, "trimesh.boolean": boolean}.items():
        sys.modules[name] = mod
    return objects


def import_reference():
    # the repo has same-named packages (src, utils, constants): the reference's must be the ones imported
    sys.path.insert(0, ROOT)
    objects = install_stubs()              # imports tests.raster_ref from the repo
    sys.path.remove(ROOT)
    os.chdir(tempfile.gettempdir())        # the reference appends the working directory to sys.path: it must not be this repo
    sys.path.insert(0, REF)
    m = importlib.import_module("src.generation.initialize_depth")
    assert m.__file__.startswith(REF), m.__file__
    sys.path.remove(REF)
    return m, objects


def patch_scene(m, objects, assets, log):
    """Scene functions of the reference's utils/blenderproc.py replaced inside the module; its own functions wrapped to record."""
    def initialize_scene(reset=False):
        SCENE.reset()
        objects.clear()
    m.initialize_scene = initialize_scene
    m.add_light = lambda *a, **kw: None
    m.add_camera = lambda resolution, name: None
    m.set_camera_config = lambda *a, **kw: None
    m.set_render_config = lambda *a, **kw: None

    def add_assets(supercategory, category, asset_id, disable_lowres_switch_for_behave=True, place_on_floor=True):
        co, faces = assets[(supercategory, category)]
        data = types.SimpleNamespace(vertices=[types.SimpleNamespace(co=v) for v in co], polygons=[types.SimpleNamespace(vertices=f) for f in faces])
        return types.SimpleNamespace(data=data, rotation_euler=None, location=None), None, None
    m.add_assets = add_assets

    def wrap(name, record):
        inner = getattr(m, name)

        def outer(*a, **kw):
            r = inner(*a, **kw)
            record(a, kw, r)
            return r
        setattr(m, name, outer)

    wrap("compute_directional_size", lambda a, kw, r: log.update(size_verts=np.array(kw["mesh_verts"]), direction=np.array(kw["direction"]), directional_size=float(r)))
    wrap("compute_nearest_point", lambda a, kw, r: log.update(asset_verts=np.array(kw["asset_verts"]), pelvis=np.array(kw["point"]),
                                                              nearest_point=np.array(r[0]), distance_from_point=float(r[1])))
    wrap("extract_candidates", lambda a, kw, r: log.update(human_verts=np.array(a[0]), human_faces=np.array(a[1]), asset_faces=np.array(a[3]),
                                                           displacements=np.array(kw["displacements"]),
                                                           cand_verts=np.stack([c["verts"] for c in r]),
                                                           cand_disp=np.stack([c["displacement"] for c in r])))
    inner_select = m.select_human

    def select_human(candidates, camera_data, gt):
        SCENE.asset = (log["asset_verts"], log["asset_faces"].astype(np.int32))
        SCENE.camera = camera_data
        del SCENE.renders[:], COUNTS[:]
        r = inner_select(candidates, camera_data, gt)
        vis = np.array(SCENE.renders, dtype=np.int64)
        inter, uni, it = np.zeros_like(vis), np.zeros_like(vis), iter(COUNTS)
        for k in np.nonzero(vis)[0]:
            inter[k], uni[k] = next(it), next(it)
        log.update(visible=vis, inter=inter, uni=uni)
        return r
    m.select_human = select_human


def disk(cx, cy, r, dtype=bool):
    yy, xx = np.mgrid[0:RES, 0:RES]
    d = (xx + 0.5 - cx) ** 2 + (yy + 0.5 - cy) ** 2 <= r * r
    return d if dtype is bool else (d * 255).astype(np.uint8)


def make_cases():
    from tests import raster_ref as RR
    rng = np.random.default_rng(20240607)
    cases = []

    def camera(eye, target, scale, obj_R=np.eye(3), obj_t=np.zeros((3, 1))):
        return dict(R=RR.look_at(eye, target), t=np.asarray(eye, dtype=np.float64), scale=float(scale), resolution=(RES, RES),
                    obj_euler=(0.0, 0.0, 0.0), obj_location=(0.0, 0.0, 0.0), obj_R=np.asarray(obj_R, dtype=np.float64), obj_t=np.asarray(obj_t, dtype=np.float64))

    def human(cx, cy, r, squash=(1.0, 1.3, 0.8), sub=2):
        v, f = RR.icosphere(sub)
        v = v * (r * np.asarray(squash)) + rng.normal(scale=0.02 * r, size=v.shape) + np.array([cx, cy, 0.0])
        return dict(verts=v, faces=f.astype(np.int64), pelvis=np.array([cx, cy + 0.2 * r, 0.0]))

    rot = RR.look_at((0.3, -1.0, 0.4))     # some rotation for obj_R
    box = RR.box((-0.45, -0.3, -0.35), (0.4, 0.35, 0.3))
    plate = RR.box((-0.9, -0.9, -0.02), (0.1, 0.9, 0.02))       # upright after the asset transform, facing the camera
    wall = RR.box((-1.0, -0.5, -0.02), (1.0, 1.5, 0.02))
    # a: box asset that hides part of the human for the far candidates; person mask = a shifted disk
    cases.append(dict(tag="a", sc="BEHAVE", c="backpack", asset=box, cam=camera((2.5, -1.0, 1.2), (0.0, 0.0, 0.4), 3.0, rot, [[0.1], [0.0], [0.2]]),
                      pred=human(30.0, 33.0, 11.0), gt=disk(31.5, 32.0, 12.0), kw=dict(interval_ratio=0.3, retrieval_range=3)))
    # b: a thin plate; the candidates in front of it tie at IoU 1 against the full silhouette (filled in below), those behind lose
    cases.append(dict(tag="b", sc="Chair", c="Lounge Chair / Cafe Chair / Office Chair", asset=plate, cam=camera((0.0, -3.0, 0.6), (0.0, 0.0, 0.5), 2.6),
                      pred=human(34.0, 30.0, 9.0), gt="silhouette", kw=dict(interval_ratio=0.3, retrieval_range=3)))
    # c: the human lies outside the image: no candidate is visible
    cases.append(dict(tag="c", sc="BEHAVE", c="backpack", asset=box, cam=camera((2.5, -1.0, 1.2), (0.0, 0.0, 0.4), 3.0),
                      pred=human(130.0, -40.0, 10.0), gt=disk(32.0, 32.0, 10.0, np.uint8), kw=dict(interval_ratio=0.3, retrieval_range=3)))
    # d: a wall that hides the candidates behind it entirely (they are skipped); 8-bit mask; another range
    cases.append(dict(tag="d", sc="INTERCAP", c="suitcase", asset=wall, cam=camera((0.4, -3.0, 0.8), (0.0, 0.0, 0.6), 3.2, np.eye(3), [[0.0], [0.0], [0.1]]),
                      pred=human(32.0, 30.0, 7.0, (1.0, 1.0, 0.6)), gt=disk(33.0, 29.0, 8.0, np.uint8), kw=dict(interval_ratio=0.45, retrieval_range=2)))
    return cases


ASSET_IDS = {"BEHAVE": "behave_asset", "Chair": "0a5a346c-cc3b-4280-b358-ccd1c4d8a865", "INTERCAP": "intercap_asset"}


def write_tree(root, case):
    sc_str, c_str, asset = case["sc"].replace("/", ":"), case["c"].replace("/", ":"), ASSET_IDS[case["sc"]]
    view, mask, prompt, iid = "view:00000", "mask:000", "a person, full body", "00000"
    os.makedirs(f"{root}/inpaint/{sc_str}/{c_str}/{asset}/{view}/{mask}/{prompt}", exist_ok=True)
    from PIL import Image              # the reference opens the picture even when the camera pickle carries the resolution
    Image.new("RGB", (RES, RES)).save(f"{root}/inpaint/{sc_str}/{c_str}/{asset}/{view}/{mask}/{prompt}/{iid}.png")
    os.makedirs(f"{root}/cam/{sc_str}/{c_str}/{asset}", exist_ok=True)
    with open(f"{root}/cam/{sc_str}/{c_str}/{asset}/{view}.pickle", "wb") as h:
        pickle.dump(case["cam"], h)
    d = f"{root}/pred/{sc_str}/{c_str}/{asset}/{view}/{mask}/{prompt}"
    os.makedirs(d, exist_ok=True)
    pred = dict(verts=case["pred"]["verts"].copy(), faces=case["pred"]["faces"].copy(), pelvis=case["pred"]["pelvis"].copy(),
                kps_aux=dict(mask_person_list=[case["gt"]]))
    with open(f"{d}/{iid}.pickle", "wb") as h:
        pickle.dump(pred, h)
    return f"{root}/save/{sc_str}/{c_str}/{asset}/{view}/{mask}/{prompt}/{iid}.pickle"


def run_reference(m, case, log):
    root = tempfile.mkdtemp(prefix="g19_")
    try:
        save_path = write_tree(root, case)
        with contextlib.redirect_stdout(io.StringIO()):
            m.initialize_depth(supercategories=None, categories=None, prompts=None, inpaint_dir=f"{root}/inpaint", camera_dir=f"{root}/cam",
                               human_pred_dir=f"{root}/pred", human_prefilter_dir=None, save_dir=f"{root}/save", kernel_size=9, max_collisions=1000,
                               parallel_num=1, parallel_idx=0, disable_lowres_switch_for_behave=False, no_initialize=False, skip_done=False,
                               verbose=False, **case["kw"])
        with open(save_path, "rb") as h:
            return pickle.load(h)
    finally:
        shutil.rmtree(root)


def main():
    m, objects = import_reference()
    sys.path.insert(0, ROOT)
    from tests import raster_ref as RR
    out, tags, log, assets = {}, [], {}, {}
    patch_scene(m, objects, assets, log)
    for case in make_cases():
        log.clear(), assets.clear()
        assets[(case["sc"], case["c"])] = case["asset"]
        if isinstance(case["gt"], str):                  # the full silhouette of the human: needs the reference's world-space verts
            run_reference(m, dict(case, gt=disk(32, 32, 5)), log)
            cam = case["cam"]
            case["gt"] = RR.raster_depth(log["human_verts"], log["human_faces"], cam["R"], cam["t"], cam["scale"], RES, RES) != RR.EMPTY
            log.clear()
        saved = run_reference(m, case, log)
        t, cam = case["tag"], case["cam"]
        tags.append(t)
        for k in ("R", "t", "obj_R", "obj_t"):
            out[f"{t}_cam_{k}"] = np.asarray(cam[k], dtype=np.float64)
        out[f"{t}_cam_scale"] = np.float64(cam["scale"])
        out[f"{t}_cam_resolution"] = np.array(cam["resolution"], dtype=np.int64)
        out[f"{t}_category"] = np.array([case["sc"], case["c"], ASSET_IDS[case["sc"]]])
        out[f"{t}_params"] = np.array([case["kw"]["interval_ratio"], case["kw"]["retrieval_range"]], dtype=np.float64)
        out[f"{t}_pred_verts"], out[f"{t}_pred_faces"], out[f"{t}_pred_pelvis"] = case["pred"]["verts"], case["pred"]["faces"], case["pred"]["pelvis"]
        out[f"{t}_gt"] = case["gt"]
        out[f"{t}_asset_co"], out[f"{t}_asset_polygons"] = case["asset"][0], case["asset"][1].astype(np.int64)
        for k, v in log.items():
            out[f"{t}_{k}"] = v
        if isinstance(saved, str):
            out[f"{t}_saved"] = np.array(saved)
            assert int(log["visible"].sum()) == 0
        else:
            out[f"{t}_sel_idx"] = np.int64(saved["idx"])
            out[f"{t}_sel_IoU"] = np.float64(saved["IoU"])
            out[f"{t}_sel_interval"] = np.int64(saved["interval_from_center"])
            out[f"{t}_sel_segmentation"] = saved["human_segmentation"]
            out[f"{t}_sel_displacement"] = np.asarray(saved["displacement"])
            out[f"{t}_sel_verts"] = np.asarray(saved["verts"])
            assert sorted(saved) == sorted(["idx", "verts", "faces", "IoU", "human_segmentation", "interval_from_center", "displacement"])
        iou = [f"{i}/{u}" for i, u in zip(log["inter"], log["uni"])]
        print(f"case {t}: visible {log['visible'].tolist()} inter/union {iou} -> {saved if isinstance(saved, str) else (saved['idx'], saved['IoU'])}")
    out["cases"] = np.array(tags)
    pth = os.path.join(HERE, "depth_init_golden.npz")
    np.savez_compressed(pth, **out)
    print(f"wrote {pth} ({os.path.getsize(pth) / 1e3:.0f} kB)")


if __name__ == "__main__":
    main()
