"""CPU-only tests of how _lib.call / _lib.query marshal their arguments from the parsed prototypes: which forms a pointer parameter
accepts, that a tensor made inside the argument list lives until the C function has returned, what is refused, and the bf16x3 routing.
The loaded library is replaced by a stand-in whose entry points are Python callables (prototypes from the real header), so nothing here
needs a built library or a device."""
import ctypes
import weakref

import pytest
import torch

from transformer_cnn_hybrid_network_for_video_processing_amd import _lib

LINEAR = "hyb_linear_fwd"          # (int dtype, x, int ldx, W, bias, y, int M, int N, int K, int flag, stream)
ENCODER = "hyb_encoder_fwd"        # (int dtype, x, mask, const float* const* params, out, saved, 6 ints, 2 floats, seed, seed_inc, stream)


class StandIn:
    """In place of the ctypes library: every attribute is a function that records its arguments, runs `probe` on them and returns 0."""

    def __init__(self, probe=None):
        self.calls, self.probe = [], probe

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if self.probe is not None:
                self.probe(args)
            return 0
        return fn


def stand_in_lib(probe=None):
    lib = _lib._Lib("unused.so")
    lib._dll = StandIn(probe)
    return lib


def watched(t, refs):
    """A temporary of the caller's argument list, observable afterwards without keeping it alive."""
    refs.append(weakref.ref(t))
    return t


def test_prototypes_used_here():
    protos = _lib.parse_header()
    assert protos[LINEAR][1] == ["int", "ptr", "int", "ptr", "ptr", "ptr", "int", "int", "int", "int", "ptr"]
    assert protos[ENCODER][1][:6] == ["int", "ptr", "ptr", "ptr", "ptr", "ptr"] and len(protos[ENCODER][1]) == 17


def test_pointer_parameter_forms():
    lib = stand_in_lib()
    x, w, y = torch.zeros(4, 8), torch.ones(3, 8), torch.empty(4, 3)
    table = (ctypes.c_void_p * 2)(5, 7)
    lib.call(LINEAR, 0, x, 8, w, None, y, 4, 3, 8, 0, 0x1234)
    lib.call(LINEAR, 0, x.data_ptr(), 8, table, None, y, 4, 3, 8, 0, None)
    (_, a), (_, b) = lib._dll.calls
    assert a == (0, x.data_ptr(), 8, w.data_ptr(), None, y.data_ptr(), 4, 3, 8, 0, 0x1234)
    assert all(type(v) is int for v in (a[1], a[3], a[5]))
    assert b[1] == x.data_ptr() and b[3] is table and b[4] is None and b[10] is None
    assert lib.query(LINEAR, 1, x, 8, w, w[0], y, 4, 3, 8, 1, None) == 0              # query marshals the same way
    assert lib._dll.calls[2][1][4] == w[0].data_ptr()


def test_list_of_tensors_becomes_an_address_array():
    lib = stand_in_lib()
    x = torch.zeros(2, 4, 8)
    ps = [torch.zeros(8, 8), torch.zeros(8), torch.zeros(3)]
    lib.call(ENCODER, 0, x, None, ps, x, x, 2, 4, 8, 16, 1, 2, 0.0, 0.0, 7, None, None)
    lib.call(ENCODER, 0, x, None, (ps[0], None, ps[2]), x, x, 2, 4, 8, 16, 1, 2, 0.0, 0.0, 7, None, None)
    arr, arr2 = lib._dll.calls[0][1][3], lib._dll.calls[1][1][3]
    assert isinstance(arr, ctypes.Array) and arr._type_ is ctypes.c_void_p
    assert list(arr) == [p.data_ptr() for p in ps]
    assert list(arr2) == [ps[0].data_ptr(), None, ps[2].data_ptr()]


def test_temporary_lives_until_the_function_returns():
    seen, refs = {}, []

    def probe(args):
        t = refs[0]()
        seen["alive"] = t is not None
        seen["addr"] = t.data_ptr() if t is not None else None
        seen["got"] = args[3]

    lib = stand_in_lib(probe)
    base, x, y = torch.arange(24.0).reshape(8, 3), torch.zeros(4, 8), torch.empty(4, 3)
    assert not base.t().is_contiguous()
    lib.call(LINEAR, 0, x, 8, watched(base.t().contiguous(), refs), None, y, 4, 3, 8, 0, None)
    assert seen["alive"] and seen["got"] == seen["addr"] and seen["addr"] != base.data_ptr()
    assert refs[0]() is None                                   # released once call() has returned


def test_temporary_inside_a_list_lives_until_the_function_returns():
    seen, refs = {}, []

    def probe(args):
        t = refs[0]()
        seen["alive"] = t is not None
        seen["addr"] = t.data_ptr() if t is not None else None
        seen["got"] = list(args[3])

    lib = stand_in_lib(probe)
    base, x, b = torch.arange(64.0).reshape(8, 8), torch.zeros(2, 4, 8), torch.zeros(8)
    lib.call(ENCODER, 0, x, None, [b, watched(base.t().contiguous(), refs)], x, x, 2, 4, 8, 16, 1, 2, 0.0, 0.0, 7, None, None)
    assert seen["alive"] and seen["got"] == [b.data_ptr(), seen["addr"]] and seen["addr"] != base.data_ptr()
    assert refs[0]() is None


def test_refusals_do_not_reach_the_function():
    lib = stand_in_lib()
    base, x, y = torch.arange(24.0).reshape(8, 3), torch.zeros(4, 8), torch.empty(4, 3)
    with pytest.raises(ValueError, match=rf"{LINEAR}: argument 3 .*not contiguous"):
        lib.call(LINEAR, 0, x, 8, base.t(), None, y, 4, 3, 8, 0, None)
    with pytest.raises(ValueError, match=rf"{ENCODER}: argument 3 .*not contiguous"):
        lib.call(ENCODER, 0, x, None, [y, base.t()], x, x, 2, 4, 8, 16, 1, 2, 0.0, 0.0, 7, None, None)
    with pytest.raises(ValueError, match=LINEAR):
        lib.query(LINEAR, 0, x, 8, base.t(), None, y, 4, 3, 8, 0, None)
    with pytest.raises(TypeError, match=rf"{LINEAR}: argument 2 is a `int` parameter"):
        lib.call(LINEAR, 0, x, torch.tensor(8), base, None, y, 4, 3, 8, 0, None)
    with pytest.raises(TypeError, match=rf"{ENCODER}: argument 12 is a `float` parameter"):
        lib.call(ENCODER, 0, x, None, [y], x, x, 2, 4, 8, 16, 1, 2, torch.zeros(()), 0.0, 7, None, None)
    with pytest.raises(TypeError, match=LINEAR):                # an argument short
        lib.call(LINEAR, 0, x, 8, base, None, y, 4, 3, 8, 0)
    assert lib._dll.calls == []


def test_mux_routes_split_bf16_calls_with_tensors():
    mux = _lib._Mux()
    mux._dll, mux.x3._dll = StandIn(), StandIn()
    x, w, y = torch.zeros(4, 8), torch.ones(3, 8), torch.empty(4, 3)
    mux.call(LINEAR, _lib.HYB_F32X3, x, 8, w, None, y, 4, 3, 8, 0, None)
    assert mux._dll.calls == []
    assert mux.x3._dll.calls == [(LINEAR, (_lib.HYB_F32, x.data_ptr(), 8, w.data_ptr(), None, y.data_ptr(), 4, 3, 8, 0, None))]
    mux.call(LINEAR, _lib.HYB_BF16, x, 8, w, None, y, 4, 3, 8, 0, None)
    assert mux._dll.calls == [(LINEAR, (_lib.HYB_BF16, x.data_ptr(), 8, w.data_ptr(), None, y.data_ptr(), 4, 3, 8, 0, None))]
    assert len(mux.x3._dll.calls) == 1


def test_loss_operator_schemas_are_the_recorded_ones():
    """The 26 hybrid::cross_entropy* / hybrid::temporal* operators -- hybrid::temporal[_bwd] and the four of every row of ops.LOSS_FAMILIES:
    each schema (argument names, types, order and defaults) equals its line of tests/golden/loss_operator_schemas.txt."""
    import os
    from transformer_cnn_hybrid_network_for_video_processing_amd import ops
    golden = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_operator_schemas.txt")).read().splitlines()
    names = [line[len("hybrid::"):line.index("(")] for line in golden]
    built = ["temporal", "temporal_bwd"] + [stem + fam.sfx + way for fam in ops.LOSS_FAMILIES.values()
                                            for stem in ("cross_entropy", "temporal_ce") for way in ("", "_bwd")]
    assert len(set(names)) == 26 and sorted(names) == sorted(built)           # none gone, none new
    assert [str(getattr(torch.ops.hybrid, n).default._schema) for n in names] == golden
