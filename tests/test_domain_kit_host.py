"""CPU checks of tests/domain_kit.py, on tiny buffers (4 x 8 with ld = 12): check_written passes a correctly written buffer and fails each
way a launch can break the contract, with the letter of the check; check_refusals fails on an accepted row and on a wrong text;
device_guard ends the session on a launch error and fails the case alone on a refusal; bits, the sentinels and pack."""
import numpy as np
import pytest
import torch

from coma_amd import _lib
from coma_amd._lib import ComaHipError
from tests import domain_kit as kit

F16, F32, F64 = torch.float16, torch.float32, torch.float64
G = kit.GUARD
O = kit.Out(4, 8, 12, F16)


def written(value=1.5):
    """(first, second, start, must, may) of a launch that wrote every owned element of O and nothing else"""
    start = kit.new_out(O)
    first = start.clone()
    kit.body(O, first)[:] = value
    return (first, first.clone(), start, *kit.masks(O))


def test_check_written_passes_a_correctly_written_buffer():
    kit.check_written("out", *written())
    flat = kit.Out(1, 10, 10, F32, must=6)                      # a flat output: six elements have to be written, four more may be
    start = kit.new_out(flat)
    first = start.clone()
    first[G:G + 6] = 2.0
    kit.check_written("stats", first, first.clone(), start, *kit.masks(flat))
    first[G + 8] = 3.0
    kit.check_written("stats", first, first.clone(), start, *kit.masks(flat))
    inf = written(float("inf"))
    kit.check_written("out", *inf, finite=False)                # (a case that says its results may be infinite)


@pytest.mark.parametrize("what, letter", [("guard", "(c)"), ("gap", "(c)"), ("unwritten", "(b)"), ("inf", "(b)"), ("second", "(d)")])
def test_check_written_fails_each_broken_contract_with_its_letter(what, letter):
    first, second, start, must, may = written()
    if what == "guard":                                         # one guard element overwritten
        first[G - 1] = second[G - 1] = 0.0
    elif what == "gap":                                         # one gap column overwritten with a finite value
        first[G + 2 * 12 + 9] = second[G + 2 * 12 + 9] = 0.25
    elif what == "unwritten":                                   # one owned element left as the sentinel
        first[G + 12 + 3] = second[G + 12 + 3] = start[0]
    elif what == "inf":                                         # one owned element infinite
        first[G + 5] = second[G + 5] = float("inf")
    else:                                                       # one bit flipped in the second launch
        kit.bits(second)[G + 3 * 12 + 7] ^= 1
    with pytest.raises(AssertionError, match=r"^\(.\) ") as e:
        kit.check_written("out", first, second, start, must, may)
    assert str(e.value).startswith(letter) and "`out`" in str(e.value)


def test_check_written_holds_integer_outputs_to_their_first_bits():
    start = kit.guarded(kit.sentinel(6, torch.int32), fill=kit.sentinel_bits(torch.int32))
    must = torch.zeros(start.numel(), dtype=torch.bool)
    must[G:G + 4] = True
    first = start.clone()
    first[G:G + 4] = 7
    kit.check_written("idx", first, first.clone(), start, must, must)
    first[G + 4] = 7                                            # an element the launch does not own
    with pytest.raises(AssertionError, match=r"^\(c\)"):
        kit.check_written("idx", first, first.clone(), start, must, must)
    u8 = kit.sentinel(4, torch.uint8)                            # every u8 value is a legitimate result, the sentinel's included
    kit.check_written("mask", u8, u8.clone(), u8.clone(), torch.ones(4, dtype=torch.bool), torch.ones(4, dtype=torch.bool))


class StubLib:
    """A "library" of one entry point that accepts what `accepts` says and reports `text` for everything else."""

    def __init__(self, accepts=lambda args: False, text="bad shape"):
        self.accepts, self.text, self.msg = accepts, text, b""

    def sd_softmax_f16(self, *args):
        if self.accepts(args):
            return 7                                            # past the argument checks: "fails where the launch needs a device"
        self.msg = f"sd_softmax_f16: {self.text} (rows = {args[1]})".encode()
        return kit.COMA_E_INVALID

    def coma_last_error(self):
        return self.msg


SOFTMAX = dict(x=kit.PTR, rows=2, n=8, ld=8, scale=1.0)
ROWS = {"sd_softmax_f16": (SOFTMAX, [("bad shape", dict(rows=0)), ("bad shape", dict(n=0))])}


def test_check_refusals_counts_the_rows_and_fails_on_an_accepted_row_and_on_a_wrong_text():
    assert _lib.PARAMS["sd_softmax_f16"] == ("x", "rows", "n", "ld", "scale", "stream")
    resolve = kit.host_resolver() if not torch.cuda.is_available() else (lambda name: 0x1000)
    base_only = lambda args: args[1] == 2 and args[2] == 8
    assert kit.check_refusals(StubLib(base_only), ROWS, resolve, expect_control=True) == 2
    with pytest.raises(AssertionError):                         # a row wrongly accepted
        kit.check_refusals(StubLib(lambda args: args[2] == 8), ROWS, resolve, expect_control=False)
    with pytest.raises(AssertionError):                         # the code is right, the text is another
        kit.check_refusals(StubLib(base_only, text="null pointer"), ROWS, resolve, expect_control=False)
    with pytest.raises(AssertionError):                         # the control: a base row that is itself refused proves nothing about the rows
        kit.check_refusals(StubLib(), ROWS, resolve, expect_control=True)
    # call(): PTR is resolved by name, Off moves it, everything else is passed as it stands, the stream is NULL
    seen = []
    lib = StubLib(lambda args: seen.append(args) or True)
    assert kit.call(lib, "sd_softmax_f16", dict(SOFTMAX, x=kit.Off(6)), lambda name: 4096) == 7 and seen == [(4102, 2, 8, 8, 1.0, None)]
    assert kit.host_resolver(("x",))("x") != kit.host_resolver()("x")         # an argument read on the host gets host memory of its own


def test_device_guard_ends_the_session_on_a_launch_error_and_fails_the_case_on_a_refusal():
    with pytest.raises(pytest.exit.Exception) as e:
        with kit.device_guard("case-12"):
            raise RuntimeError("HIP error: an illegal memory access was encountered")
    assert e.value.returncode == 3 and "case-12: RuntimeError: HIP error" in str(e.value)
    with pytest.raises(pytest.exit.Exception):                  # another code of the library is no refusal
        with kit.device_guard("case-13"):
            raise ComaHipError("sd_softmax_f16 failed (-3): launch failed")
    with pytest.raises(ComaHipError, match=r"failed \(-1\)"):
        with kit.device_guard("case-14"):
            raise ComaHipError(f"sd_softmax_f16 failed ({kit.COMA_E_INVALID}): sd_softmax_f16: bad shape")
    with pytest.raises(pytest.fail.Exception):                  # the C-ABI variant: a refused case fails, the session goes on
        with kit.device_guard("case-15"):
            pytest.fail("refused inside the accepted domain")
    with pytest.raises(pytest.exit.Exception):                  # launch_twice stands on the same guard
        kit.launch_twice(dict, lambda bufs: 1 / 0, "case-16")


def test_bits_round_trips_every_type_the_suites_use():
    for dt, width in ((F16, torch.int16), (F32, torch.int32), (F64, torch.int64)):
        t = torch.tensor([1.5, -0.0, float("nan"), float("inf")], dtype=dt)
        b = kit.bits(t)
        assert b.dtype == width and torch.equal(kit.bits(b.view(dt)), b) and int(b[1]) != 0 and int(kit.bits(kit.sentinel(1, dt))[0]) == kit.sentinel_bits(dt)
    for dt in (torch.uint8, torch.int32, torch.int64):
        t = torch.tensor([0, 1, 100], dtype=dt)
        assert kit.bits(t) is t
    for dt, width in ((np.float16, np.uint16), (np.float32, np.uint32), (np.float64, np.uint64)):
        a = np.array([1.5, -0.0, np.nan, np.inf], dtype=dt)
        b = kit.bits(a)
        assert b.dtype == width and np.array_equal(b.view(dt).view(width), b) and b[1] != 0 and kit.bits(kit.sentinel(1, dt))[0] == kit.sentinel_bits(dt)
    for dt in (np.uint8, np.int32, np.int64):
        a = np.array([0, 1, 100], dtype=dt)
        assert np.array_equal(kit.bits(a), a) and kit.bits(a).dtype == dt


def test_the_sentinels_are_nans_and_pack_leaves_nothing_but_nan_around_the_data():
    assert (kit.sentinel_bits(F16), kit.sentinel_bits(F32), kit.sentinel_bits(F64)) == (0x7E5A, 0x7FC5A5A5, 0x7FF8A5A5A5A5A5A5)
    assert (kit.sentinel_bits(np.uint8), kit.sentinel_bits(np.int32) & 0xFFFFFFFF, kit.sentinel_bits(np.int64) & (2 ** 64 - 1)) == \
        (0xA5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5)
    for dt in (F16, F32, F64, np.float16, np.float32, np.float64):
        s = kit.sentinel(5, dt)
        assert len(s) == 5 and bool(np.isnan(np.asarray(s)).all())
    assert kit.COMA_E_INVALID == -1 and kit.device_bound(0.0) == kit.FLOOR == 2.0 ** -10 and kit.device_bound(1e-3) == 4e-3 and kit.device_bound(0.0, 5 * kit.U32) == 5 * kit.U32
    op = kit.Operand(torch.arange(32, dtype=F16).view(4, 8), 12, off=4)
    buf = kit.pack(op)
    data = torch.zeros(buf.numel(), dtype=torch.bool)
    data[G + 4:G + 4 + 4 * 12].view(4, 12)[:, :8] = True
    assert buf.numel() == G + 4 + 4 * 12 + G and torch.equal(buf[data].view(4, 8), op.t) and bool(buf[~data].isnan().all())
    rows = kit.pack_rows(np.arange(32, dtype=np.float32).reshape(4, 8), np.nan, ld=12, off=4)
    assert np.array_equal(rows, buf.float().numpy(), equal_nan=True) and int(np.isnan(rows).sum()) == 2 * G + 4 + 4 * 4
    ids = kit.pack_rows(np.arange(6, dtype=np.int32), 0x7FFFFFFF)             # integers: the poison the caller names
    assert ids.size == 6 + 2 * G and (ids[:G] == 0x7FFFFFFF).all() and (ids[-G:] == 0x7FFFFFFF).all() and np.array_equal(ids[G:-G], np.arange(6))
