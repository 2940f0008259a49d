#!/usr/bin/env python3
"""Golden vectors for the sample metrics and the post-filter, produced by the REAL reference modules
(/root/reference/src/generation/compute_metrics.py and src/coma/filter.py) with Blender, trimesh and cv2 stubbed out (the stand-ins
of make_golden_depth_init.py).

Recorded, all from the reference's own code:
  * get_asset_info for one category of each dataset type (`trimesh.load` is a stand-in that hands back the synthetic OBJ vertices);
  * save_human end to end on one BEHAVE sample with `compute_metrics` -- the Blender boolean and render -- replaced by fixed numbers:
    the pickle keys and the frame change of :240-241;
  * save_human on a tree of sentinel pickles for several (parallel_num, parallel_idx): which files each process writes;
  * run_post_filtering on a synthetic tree of sample pickles, in both prompt modes: every JSON file and the printed summary.
Only data is stored: arrays, names, the pickles' contents as JSON text, and the texts the reference wrote.

Writes tests/golden/metrics_golden.npz.   Run (build container only): python tests/golden/make_golden_metrics.py
"""
import contextlib
import importlib
import io
import json
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

TYPES = [("3D-FUTURE", "Chair", "Lounge Chair / Cafe Chair / Office Chair", "0a5a346c-cc3b-4280-b358-ccd1c4d8a865"),
         ("SHAPENET", "motorcycle,bike", "motorcycle,bike", "9b9794dda0a6532215a11c390f7ca182"),
         ("SKETCHFAB", "umbrella", "umbrella", "85fto9rtgcvsx2itzy9rd0gwh7758d64"),
         ("BEHAVE", "BEHAVE", "backpack", "behave_asset"),
         ("INTERCAP", "INTERCAP", "suitcase", "intercap_asset")]
SLICES = [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (7, 0), (7, 3), (7, 6), (8, 1)]
N_SLICE_ITEMS = 7

# the filter fixture: (supercategory, category, asset, view, mask, prompt directory, id, payload); a payload is a dict or a sentinel
FILTER_TREE = [
    ("BEHAVE", "backpack", "bp0", "view:00000", "mask:000", "sitting on the backpack, full body", "00000", dict(IoU=0.9, interscetion_ratio=0.01, num_inliers=5)),
    ("BEHAVE", "backpack", "bp0", "view:00000", "mask:000", "sitting on the backpack, full body", "00001", dict(IoU=0.5, interscetion_ratio=0.01, num_inliers=5)),
    ("BEHAVE", "backpack", "bp0", "view:00000", "mask:000", "sitting on the backpack, full body", "00002", dict(IoU=0.9, interscetion_ratio=0.2, num_inliers=5)),
    ("BEHAVE", "backpack", "bp0", "view:00000", "mask:001", "sitting on the backpack, full body", "00000", dict(IoU=0.9, interscetion_ratio=0.01, num_inliers=0)),
    ("BEHAVE", "backpack", "bp0", "view:00001", "mask:000", "sitting on the backpack, full body", "00000", dict(IoU=0.8, interscetion_ratio=0.03)),
    ("BEHAVE", "backpack", "bp0", "view:00001", "mask:000", "sitting on the backpack, full body", "00001", "NO HUMANS"),
    ("BEHAVE", "backpack", "bp0", "view:00001", "mask:000", "sitting on the backpack, upper body", "00000", dict(IoU=0.95, interscetion_ratio=0.0, num_inliers=9)),
    ("BEHAVE", "backpack", "bp0", "view:00001", "mask:000", "carrying the backpack", "00000", dict(IoU=0.7, interscetion_ratio=0.05, num_inliers=1)),
    ("BEHAVE", "backpack", "bp0", "view:00001", "mask:000", "carrying the backpack", "00001", dict(IoU=0.1, interscetion_ratio=0.9, num_inliers=0)),
    ("BEHAVE", "backpack", "bp0", "view:00001", "mask:000", "a person carrying the backpack, full body", "00000", dict(IoU=0.9, interscetion_ratio=0.01, num_inliers=5)),
    ("INTERCAP", "suitcase", "sc0", "view:00000", "mask:000", "pulling the suitcase, full body", "00000", dict(IoU=0.2, interscetion_ratio=0.0, num_inliers=3)),
    ("BEHAVE", "backpack", "bp0", "view:00000", "mask:000", "total:sitting on the backpack, full body", "00000", dict(IoU=0.9, interscetion_ratio=0.01, num_inliers=5)),
    ("BEHAVE", "backpack", "bp0", "view:00000", "mask:000", "total:sitting on the backpack, full body", "00001", dict(IoU=0.9, interscetion_ratio=0.06, num_inliers=5)),
    ("BEHAVE", "backpack", "bp0", "view:00001", "mask:000", "total:carrying the backpack", "00000", dict(IoU=0.75, interscetion_ratio=0.0)),
]
FILTER_KW = dict(IoU_threshold_min=0.7, intersection_volume_ratio_threshold_max=0.05, inlier_num_threshold_min=1)
FIXED_METRICS = dict(interscetion_ratio=0.0125, IoU=0.8125)


def import_reference():
    sys.path.insert(0, HERE)
    import make_golden_depth_init as G          # its stand-ins for bpy, blenderproc, cv2, trimesh, tqdm
    sys.path.remove(HERE)
    sys.path.insert(0, ROOT)
    G.install_stubs()
    sys.path.remove(ROOT)
    for name in [n for n in sys.modules if n == "tests" or n.startswith("tests.")]:
        del sys.modules[name]
    os.chdir(tempfile.gettempdir())        # the reference appends the working directory to sys.path: it must not be this repo
    sys.path.insert(0, REF)
    cm = importlib.import_module("src.generation.compute_metrics")
    flt = importlib.import_module("src.coma.filter")
    assert cm.__file__.startswith(REF) and flt.__file__.startswith(REF), (cm.__file__, flt.__file__)
    sys.path.remove(REF)
    return cm, flt


def synthetic_obj(rng, n=40):
    v = rng.normal(size=(n, 3)) * np.array([0.4, 0.7, 0.3]) + np.array([0.05, 0.3, -0.1])
    f = rng.integers(0, n, size=(60, 3))
    return v, f


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def write_tree(root, entries):
    for sc, c, asset, view, mask, prompt, iid, payload in entries:
        d = f"{root}/{sc}/{c}/{asset}/{view}/{mask}/{prompt}"
        os.makedirs(d, exist_ok=True)
        with open(f"{d}/{iid}.pickle", "wb") as h:
            pickle.dump(payload, h)


def relative_files(root, ext):
    out = []
    for d, _, files in os.walk(root):
        out += [os.path.relpath(os.path.join(d, f), root) for f in files if f.endswith(ext)]
    return sorted(out)


def main():
    cm, flt = import_reference()
    rng = np.random.default_rng(20240611)
    out = {}
    work = tempfile.mkdtemp(prefix="g20_")
    os.chdir(work)                              # the reference's dataset paths are relative: "data/..."
    try:
        # ---- get_asset_info, one category per dataset type ----
        loaded = {}
        sys.modules["trimesh"].load = lambda pth, force=None, process=None: types.SimpleNamespace(vertices=loaded[pth][0], faces=loaded[pth][1])
        os.makedirs("data/ShapeNetCore.v2")
        with open("data/ShapeNetCore.v2/taxonomy.json", "w") as h:
            json.dump([dict(name="chair", synsetId="03001627"), dict(name="motorcycle,bike", synsetId="03790512")], h)
        expected_pth = {"3D-FUTURE": "data/3D-FUTURE-model/{a}/raw_model.obj", "SHAPENET": "data/ShapeNetCore.v2/03790512/{a}/models/model_normalized.obj",
                        "SKETCHFAB": "data/SketchFab/{sc}/{a}/model.obj", "BEHAVE": "data/BEHAVE/objects/{c}/{c}_canon_lowres_in_gen_coord.obj",
                        "INTERCAP": "data/INTERCAP/objects/{c}/mesh.obj"}
        for kind, sc, c, asset in TYPES:
            v, f = synthetic_obj(rng)
            pth = expected_pth[kind].format(a=asset, sc=sc, c=c)
            loaded.clear()
            loaded[pth] = (v, f)
            cam = dict(obj_R=rotation(rng), obj_t=rng.normal(size=(3, 1)) * 0.3)
            info = cm.get_asset_info(sc, c, asset, "view:00000", cam, False)
            out[f"asset_{kind}_names"] = np.array([sc, c, asset])
            out[f"asset_{kind}_path"] = np.array(pth)
            out[f"asset_{kind}_obj_verts"], out[f"asset_{kind}_obj_faces"] = v, f
            out[f"asset_{kind}_obj_R"], out[f"asset_{kind}_obj_t"] = cam["obj_R"], cam["obj_t"]
            out[f"asset_{kind}_verts"], out[f"asset_{kind}_faces"], out[f"asset_{kind}_z_min"] = info["verts"], info["faces"], np.float64(info["z_min"])
        out["asset_types"] = np.array([t[0] for t in TYPES])

        # ---- save_human on one BEHAVE sample, the two third-party metrics replaced by fixed numbers ----
        cm.ASSET_INFO.clear()
        cm.compute_metrics = lambda *a, **kw: dict(FIXED_METRICS)
        kind, sc, c, asset = TYPES[3]
        v, f = synthetic_obj(rng)
        loaded.clear()
        loaded[f"data/BEHAVE/objects/{c}/{c}.obj"] = (v, f)            # the CLI default disable_lowres_switch_for_behave=True
        cam = dict(obj_R=rotation(rng), obj_t=rng.normal(size=(3, 1)) * 0.3, R=np.eye(3), t=np.zeros(3), scale=2.0, resolution=(32, 32))
        human = dict(verts=rng.normal(size=(25, 3)), faces=rng.integers(0, 25, size=(30, 3)), num_inliers=4)
        prompt, iid = "sitting on the backpack, full body", "00000"
        write_tree("after_opt", [(sc, c, asset, "view:00000", "mask:000", prompt, iid, human)])
        os.makedirs(f"cam/{sc}/{c}/{asset}")
        with open(f"cam/{sc}/{c}/{asset}/view:00000.pickle", "wb") as h:
            pickle.dump(cam, h)
        kw = dict(supercategories=None, categories=None, prompts=None, human_pred_dir="pred", camera_dir="cam", enable_aggregate_total_prompts=False,
                  disable_lowres_switch_for_behave=True, skip_done=False)
        cm.save_human(human_after_opt_dir="after_opt", save_dir="sample", parallel_idx=0, parallel_num=1, **kw)
        with open(f"sample/{sc}/{c}/{asset}/view:00000/mask:000/{prompt}/{iid}.pickle", "rb") as h:
            saved = pickle.load(h)
        out["frame_names"] = np.array([sc, c, asset, prompt, iid])
        out["frame_obj_verts"], out["frame_obj_faces"] = v, f
        out["frame_obj_R"], out["frame_obj_t"] = cam["obj_R"], cam["obj_t"]
        out["frame_human_verts"], out["frame_human_faces"] = human["verts"], human["faces"]
        out["frame_saved_keys"] = np.array(sorted(saved))
        out["frame_saved_verts"], out["frame_saved_z_min"] = saved["verts"], np.float64(saved["z_min"])
        out["frame_saved_metrics"] = np.array([saved["interscetion_ratio"], saved["IoU"], saved["num_inliers"]], dtype=np.float64)

        # ---- the slice rule, on sentinel pickles ----
        entries = [("BEHAVE", "backpack", "bp0", f"view:{k // 3:05d}", "mask:000", "sitting on the backpack, full body", f"{k % 3:05d}", "NO HUMANS")
                   for k in range(N_SLICE_ITEMS)]
        write_tree("slice_in", entries)
        out["slice_inputs"] = np.array(relative_files("slice_in", ".pickle"))
        for num, idx in SLICES:
            dst = f"slice_out_{num}_{idx}"
            cm.save_human(human_after_opt_dir="slice_in", save_dir=dst, parallel_idx=idx, parallel_num=num, **kw)
            out[f"slice_{num}_{idx}"] = np.array(relative_files(dst, ".pickle"), dtype=str) if os.path.isdir(dst) else np.array([], dtype=str)
        out["slices"] = np.array(SLICES, dtype=np.int64)

        # ---- the post-filter ----
        write_tree("filter_in", FILTER_TREE)
        out["filter_tree_paths"] = np.array(["/".join(e[:6]) + f"/{e[6]}.pickle" for e in FILTER_TREE])
        out["filter_tree_payloads"] = np.array([json.dumps(e[7]) for e in FILTER_TREE])
        out["filter_kw"] = np.array(json.dumps(FILTER_KW))
        for mode, total in (("plain", False), ("total", True)):
            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                flt.run_post_filtering(supercategories=None, categories=None, prompts=None, human_sample_dir="filter_in", save_dir=f"filter_out_{mode}",
                                       enable_aggregate_total_prompts=total, parallel_num=1, parallel_idx=0, **FILTER_KW)
            files = relative_files(f"filter_out_{mode}", ".json")
            out[f"filter_{mode}_files"] = np.array(files)
            out[f"filter_{mode}_json"] = np.array([open(f"filter_out_{mode}/{p}").read() for p in files])
            out[f"filter_{mode}_stdout"] = np.array(text.getvalue().replace(f"filter_out_{mode}", "SAVE_DIR"))
            print(mode, files, text.getvalue().split("RESULTS ================")[1].split())
    finally:
        os.chdir(HERE)
        shutil.rmtree(work)
    pth = os.path.join(HERE, "metrics_golden.npz")
    np.savez_compressed(pth, **out)
    print(f"wrote {pth} ({os.path.getsize(pth) / 1e3:.0f} kB)")


if __name__ == "__main__":
    main()
