"""The rules of coma_amd/sd/gn_stats.py::GnStats -- which producer leaves GroupNorm statistics, which consumer may read them -- pinned as
literals (DESIGN.md 5 states the same table).  The allocator is a fake that records what was asked for: no device."""
import pytest
import torch

from coma_amd.sd.gn_stats import GnStats


class FakeAlloc:
    def __init__(self):
        self.calls = []

    def __call__(self, *shape, dtype=None, zero=False):
        self.calls.append((list(shape), dtype, zero))
        return torch.empty(*shape, dtype=dtype)          # real storage: buffers are told apart by data_ptr()


def owner(fuse=True):
    alloc = FakeAlloc()
    st = GnStats(alloc)
    st.fuse_gn_stats = fuse
    return st, alloc


def tensor():
    return torch.empty(8)


def same(got, want):
    """(colstats0, colstats1, rows per slot): the buffers by identity."""
    return got[0] is want[0] and got[1] is want[1] and got[2] == want[2]


NONE = (None, None, 32)


N = 320
# (kind, arguments of produce) -> shape of the one buffer allocated, or None
PRODUCERS = [
    ("gemm", dict(rows=16384, n=N, hw=4096, z=1), [512, 2, N]),
    ("gemm", dict(rows=16352, n=N, hw=4088, z=1), None),                  # below 16384
    ("gemm", dict(rows=16400, n=N, hw=4100, z=1), None),                  # not a multiple of 32
    ("gemm", dict(rows=16384, n=N, hw=4096, z=16), None),
    ("gemm", dict(rows=16384, n=N, hw=4096, z=1, asked=False), None),
    ("phase", dict(rows=4 * 4096, n=N, hw=4 * 1024), [512, 2, N]),        # source M = 4096, in_h * in_w = 1024
    ("phase", dict(rows=4 * 36 * 128, n=N, hw=4 * 36), None),             # in_h * in_w = 36 (18432 output rows: the row rule alone would pass)
    ("winograd", dict(rows=16384, n=640, hw=1024, w=32), [512, 2, 640]),
    ("winograd", dict(rows=16384, n=640, hw=256, w=16), None),
    ("winograd", dict(rows=16384, n=320, hw=1024, w=32), None),
    ("xtail", dict(rows=16384, n=320), [512, 2, 320]),                    # without being asked
    ("xtail", dict(rows=8192, n=320), None),
    ("tile", dict(rows=2 * 16 * 16, n=128, hw=16 * 16), [2, 2, 128]),     # halo / c3: batch 2, 16 x 16, 256-row slots
]


@pytest.mark.parametrize("kind,kw,shape", PRODUCERS)
def test_producer_rules(kind, kw, shape):
    st, alloc = owner()
    cs = st.produce(tensor(), kind, **kw)
    if shape is None:
        assert cs is None and alloc.calls == []
    else:
        assert alloc.calls == [(shape, torch.float32, True)] and list(cs.shape) == shape


@pytest.mark.parametrize("kind,kw,shape", PRODUCERS)
def test_no_producer_leaves_statistics_with_fusion_off(kind, kw, shape):
    st, alloc = owner(fuse=False)
    out = tensor()
    assert st.produce(out, kind, **kw) is None and alloc.calls == []
    assert same(st.consume(out, hw=1024, accepts=(256, 32)), NONE)


def test_phase_launches_share_one_buffer():
    """The four sub-pixel launches write one output: one produce call, one buffer, found under that output."""
    st, alloc = owner()
    out = tensor()
    cs = st.produce(out, "phase", rows=16384, n=N, hw=4096)
    assert len(alloc.calls) == 1
    assert st.consume(out, hw=4096)[0] is cs


GROUPNORM, TABLE = (32,), (256, 32)


def test_consumers_of_32_row_statistics():
    st, _ = owner()
    x = tensor()
    cs = st.produce(x, "gemm", rows=16384, n=N, hw=1024)
    for accepts in (GROUPNORM, TABLE):
        assert same(st.consume(x, hw=1024, accepts=accepts), (cs, None, 32))
        # 1296 = 36 x 36: a slot would straddle two samples -- groupnorm falls back to its statistics pass, a table consumer gets none
        assert same(st.consume(x, hw=1296, accepts=accepts), NONE)
    assert same(st.consume(tensor(), hw=1024, accepts=TABLE), NONE)       # a tensor no producer left anything for


@pytest.mark.parametrize("hw", [256, 1024, 1296])
def test_tile_statistics_reach_table_consumers_only_and_are_preferred(hw):
    st, _ = owner()
    x = tensor()
    cs32 = st.produce(x, "gemm", rows=16384, n=128, hw=1024)
    cs256 = st.produce(x, "tile", rows=16384, n=128, hw=1024)
    assert same(st.consume(x, hw=hw, accepts=TABLE), (cs256, None, 256))
    assert same(st.consume(x, hw=hw, accepts=GROUPNORM), (cs32, None, 32) if hw % 32 == 0 else NONE)
    y = tensor()
    cs = st.produce(y, "tile", rows=512, n=128, hw=256)
    assert same(st.consume(y, hw=hw, accepts=TABLE), (cs, None, 256))
    assert same(st.consume(y, hw=hw, accepts=GROUPNORM), NONE)


@pytest.mark.parametrize("hw", [1024, 1296])
def test_two_sources_need_statistics_of_both(hw):
    st, _ = owner()
    x0, x1, bare = tensor(), tensor(), tensor()
    cs0 = st.produce(x0, "gemm", rows=16384, n=N, hw=1024)
    cs1 = st.produce(x1, "xtail", rows=16384, n=320)
    usable = hw % 32 == 0
    assert same(st.consume(x0, x1, hw=hw), ((cs0, cs1, 32) if usable else NONE))
    assert same(st.consume(x1, x0, hw=hw), ((cs1, cs0, 32) if usable else NONE))
    assert same(st.consume(x0, bare, hw=hw), NONE)
    assert same(st.consume(bare, x0, hw=hw), NONE)
    # one source with 32-row slots, one with per-tile slots: no common slot size, nothing usable
    tiled = tensor()
    st.produce(tiled, "tile", rows=16384, n=N, hw=1024)
    assert same(st.consume(x0, tiled, hw=hw, accepts=TABLE), NONE)


def test_dup_carries_32_row_statistics_only():
    st, alloc = owner()
    src, dst = tensor(), tensor()
    cs = st.produce(src, "gemm", rows=16384, n=N, hw=4096)
    pair = st.follow(src, dst)
    assert pair[0] is cs and alloc.calls[-1] == ([1024, 2, N], torch.float32, True)      # twice the slots
    assert same(st.consume(dst, hw=4096), (pair[1], None, 32))
    assert same(st.consume(dst, hw=1296), NONE)
    # per-tile statistics do not follow the copy, and a source without statistics leaves none
    tsrc, tdst = tensor(), tensor()
    st.produce(tsrc, "tile", rows=512, n=128, hw=256)
    n = len(alloc.calls)
    assert st.follow(tsrc, tdst) is None and st.follow(tensor(), tensor()) is None and len(alloc.calls) == n
    assert same(st.consume(tdst, hw=256, accepts=TABLE), NONE)
