"""Asset tables of the generation stage, restated compactly (values: reference constants/generation/assets.py:1-43).
Only what src/generation/initialize_depth.py reads: where a category's meshes live and which dataset rules apply to it."""

# dataset type -> directory under --asset_obj_root (the reference's "data/<...>" with the "data" part left to the flag)
DATASET_DIRS = {
    "3D-FUTURE": "3D-FUTURE-model",
    "SHAPENET": "ShapeNetCore.v2",
    "SKETCHFAB": "SketchFab",
    "SAPIEN": "SAPIEN",
    "BEHAVE": "BEHAVE",
    "INTERCAP": "INTERCAP",
}

# (supercategory, category) -> dataset type
CATEGORY2DATASET_TYPE = {
    ("Chair", "Lounge Chair / Cafe Chair / Office Chair"): "3D-FUTURE",
    ("motorcycle,bike", "motorcycle,bike"): "SHAPENET",
    ("umbrella", "umbrella"): "SKETCHFAB",
    ("frypan", "frypan"): "SKETCHFAB",
    ("cart", "cart"): "SAPIEN",
    ("BEHAVE", "backpack"): "BEHAVE",
    ("INTERCAP", "suitcase"): "INTERCAP",
}

# dataset types whose assets are put back on the floor after the object transform (initialize_depth.py:344-345)
FLOOR_SHIFTED_DATASETS = ("SHAPENET", "SKETCHFAB", "INTERCAP", "BEHAVE")
