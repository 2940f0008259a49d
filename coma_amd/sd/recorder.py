"""The launch recorder every network of the project is built on: a flat list of kernel launches over pre-allocated buffers (no allocation,
no host sync inside), RECORDED into a library-owned model (coma_amd/csrc/sd_plan.hip, sd/model.py).  The launch list and the hipGraph
captured from it live in libcoma_hip.so, a forward is one sd_model_replay, and the model can be saved to a file a caller without Python
loads and runs.  The Python closures are kept for per-launch profiling (`run`, `profile`).  The recorder knows no operator: the diffusion
vocabulary is sd/graph.py::LaunchGraph, the segmentation plan (seg/model.py) adds its own launches.
"""
from __future__ import annotations

import torch

from .model import BUF_ZEROED, SdModel

F16 = torch.float16


class LaunchRecorder:
    def __init__(self, device, model=None, plan="step"):
        self.device = torch.device(device)
        self.model = model if model is not None else SdModel(device)     # several recorders may share one model (UNet: step + context)
        self.plan = plan
        self._recorded = False
        self.launches = []          # zero-argument closures
        self.tags = []              # (description, flops) per launch, for profiling
        self.alg_bytes = []         # algorithmic HBM bytes per launch (inputs read once + output written once)
        self.flops = 0              # ALGORITHMIC flops per run: 2*M*N*K of every GEMM-shaped operator (a Winograd convolution counts as the
                                    # 3x3 convolution it computes, 2 * 9 * M * N * C_in)
        self.exec_flops = 0         # MFMA flops actually issued (a Winograd convolution: 16 plane products = 4/9 of the above)
        self.exec_tags = []         # executed flops per launch, parallel to `tags`

    # ---- memory
    def buf(self, *shape, dtype=F16, zero=False):
        t = (torch.zeros if zero else torch.empty)(*shape, dtype=dtype, device=self.device)
        self.model.register(t, BUF_ZEROED if zero else 0)                # scratch: not part of a saved model's contents
        return t

    # ---- recording
    def add(self, fn, flops=0, tag="", nbytes=0, alg_flops=None):
        alg = flops if alg_flops is None else alg_flops
        self.launches.append(fn)
        self.tags.append((tag, alg))
        self.exec_tags.append(flops)
        self.alg_bytes.append(nbytes)
        self.flops += alg
        self.exec_flops += flops

    # ---- execution
    def run(self):
        for fn in self.launches:
            fn()

    def execute(self, use_graph=True):
        """One forward: the library's hipGraph of the recorded list, or the Python closures one by one."""
        if use_graph:
            self.replay()
        else:
            self.run()

    def profile(self, reps=3):
        """Eager per-launch timing with HIP events -> list of (tag, flops, ms); for tuning only."""
        dev = self.device
        self.run()
        torch.cuda.synchronize(dev)
        out = []
        for fn, (tag, fl) in zip(self.launches, self.tags):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize(dev)
            out.append((tag, fl, a.elapsed_time(b) / reps))
        return out

    def capture(self):
        """Record the launch list into the library-owned plan (once), run it eagerly once (module loading and argument checks happen
        outside any capture); the library captures its hipGraph on the first replay."""
        if not self._recorded:
            def record_checked():
                # every closure must end up in the plan: one that calls no library entry point (a stray torch op) would execute now,
                # during recording, and be missing from every replay and from a saved model
                for fn, (tag, _) in zip(self.launches, self.tags):
                    n0 = self.model.num_launches(self.plan)
                    fn()
                    if self.model.num_launches(self.plan) <= n0:
                        raise RuntimeError(f"launch '{tag}' of plan '{self.plan}' recorded nothing: only recordable entry points of the library may be added")
            assert len(self.tags) == len(self.launches)
            self.model.record(self.plan, record_checked)
            self._recorded = True
            self.model.run(self.plan)
            torch.cuda.synchronize(self.device)
        return self.model

    def run_recorded(self):
        """The recorded list launched natively one by one (no Python per launch, no graph)."""
        self.capture()
        self.model.run(self.plan)

    def replay(self):
        if not self._recorded:
            self.capture()            # recorded, then run eagerly once: that run IS this call's execution (no second pass over the step)
            self.model.prepare(self.plan)      # the hipGraph is captured and instantiated now (nothing executes), so the next call only launches
            return
        self.model.replay(self.plan)
