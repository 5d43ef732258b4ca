"""The host side of the conv-net and MLP C calls, without a GPU: the one weight packer against a plain loop, the
"parameters changed" memo, the head arrays of the `_head` Sequential, the default trio's weight-struct keeper and the
device-ordinal helper."""
import pytest
import torch

import muax_amd as mx
from muax_amd import _call, _lib

nn_ = mx.nn
CASES = [(4, 16), (16, 16), (32, 64), (33, 32), (65, 64)]  # (Cin, Cout); 33 and 65: the EZ stem's C + 1


def _pad16(cin):
    return -(-cin // 16) * 16


def _loop_pack(w, cin_pad):
    """Wp[tap][c][g][co][i] = W[tap][16 c + 4 g + i][co], zero for rows past Cin: the layout as the kernels state it."""
    cin, cout = w.shape[2], w.shape[3]
    w9 = w.reshape(9, cin, cout)
    out = torch.zeros(9, cin_pad // 16, 4, cout, 4)
    for tap in range(9):
        for c in range(cin_pad // 16):
            for g in range(4):
                for co in range(cout):
                    for i in range(4):
                        row = 16 * c + 4 * g + i
                        if row < cin:
                            out[tap, c, g, co, i] = w9[tap, row, co]
    return out


def _hwio(cin, cout, seed=0):
    return torch.randn(3, 3, cin, cout, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def resnet():
    """A CPU-materialised ResNetPrediction / ResNetDynamic pair at the width the kernels are built for."""
    g = torch.Generator().manual_seed(3)
    pred, dyn = nn_.ResNetPrediction(18, 21, generator=g), nn_.ResNetDynamic(18, 21, generator=g)
    s = torch.rand(2, 6, 6, 64, generator=g)
    with torch.no_grad():
        pred(s)
        dyn(s, torch.tensor([1, 17]))
    return pred, dyn


@pytest.fixture(scope="module")
def ez():
    g = torch.Generator().manual_seed(4)
    pred, dyn = nn_.EZPrediction(6, 21, 0.1, generator=g), nn_.EZDynamic(32, 6, 21, 0.1, generator=g)
    s = torch.rand(2, 6, 6, 32, generator=g)
    with torch.no_grad():
        pred(s)
        dyn(s, torch.tensor([0, 5]))
    return pred, dyn


# ---- packers ----
@pytest.mark.parametrize("cin,cout", CASES)
def test_pack_conv3x3_is_the_loop(cin, cout):
    w = _hwio(cin, cout)
    assert torch.equal(nn_.pack_conv3x3(w, _pad16(cin)), _loop_pack(w, _pad16(cin)))
    if cin % 16 == 0:
        assert torch.equal(nn_.pack_conv3x3(w), _loop_pack(w, cin))
    assert nn_.pack_conv3x3(w, _pad16(cin)).is_contiguous()


@pytest.mark.parametrize("cin,cout", CASES)
def test_hkconv2d_packed_is_the_loop(cin, cout):
    conv = nn_.HkConv2D(cout, 3, 1, in_channels=cin, generator=torch.Generator().manual_seed(1))
    assert torch.equal(conv._packed(), _loop_pack(conv.w.detach(), _pad16(cin)))


def test_ez_packed_convs_are_the_loop(ez):
    pred, dyn = ez
    pk = dyn._ez_packed(pred)
    assert torch.equal(pk["d_conv"], _loop_pack(dyn.conv.w.detach(), 32 + 16))  # 33 rows in a width of C + 16
    for name, conv in (("d_conv0", dyn.block.conv_0), ("d_conv1", dyn.block.conv_1),
                       ("p_conv0", pred.block.conv_0), ("p_conv1", pred.block.conv_1)):
        assert torch.equal(pk[name], _loop_pack(conv.w.detach(), 32))


def test_tower_packed_convs_are_the_loop(resnet):
    _, dyn = resnet
    stem, conv, ln = dyn._packed()
    assert tuple(conv.shape) == (8, 3, 9, 4, 4, 64, 4) and conv.is_contiguous()
    for b in (0, 7):
        blk = dyn.ns_blocks[b]
        for j, m in enumerate((blk.proj_conv, blk.conv_0, blk.conv_1)):
            assert torch.equal(conv[b][j], _loop_pack(m.w.detach(), 64))
    assert torch.equal(stem, dyn.ns_stem.w.detach().reshape(65, 64))
    assert torch.equal(ln[3][1], torch.stack([dyn.ns_blocks[3].ln_0.scale, dyn.ns_blocks[3].ln_0.offset]).detach())


# ---- memo ----
def test_packed_is_kept_until_the_parameter_is_written_or_moved():
    conv = nn_.HkConv2D(16, 3, 1, in_channels=16, generator=torch.Generator().manual_seed(2))
    p0 = conv._packed()
    assert conv._packed() is p0
    with torch.no_grad():
        conv.w.add_(1)  # _version
    p1 = conv._packed()
    assert p1 is not p0 and torch.equal(p1, _loop_pack(conv.w.detach(), 16))
    assert conv._packed() is p1
    conv.w.data = conv.w.data.clone()  # pointer
    p2 = conv._packed()
    assert p2 is not p1 and torch.equal(p2, p1) and conv._packed() is p2


def test_oihw_is_kept_in_inference_and_a_differentiable_view_in_training():
    conv = nn_.HkConv2D(16, 3, 1, in_channels=16, generator=torch.Generator().manual_seed(2))
    assert conv._oihw()._base is conv.w  # training: the view autograd follows
    with torch.no_grad():
        o0 = conv._oihw()
        assert conv._oihw() is o0 and torch.equal(o0, conv.w.permute(3, 2, 0, 1))
        conv.w.add_(1)
        assert conv._oihw() is not o0 and torch.equal(conv._oihw(), conv.w.permute(3, 2, 0, 1))


def test_tower_and_ez_packs_follow_their_parameters(resnet, ez):
    _, dyn = resnet
    p0 = dyn._packed()
    assert dyn._packed() is p0
    with torch.no_grad():
        dyn.ns_blocks[5].ln_1.offset.add_(1)
    assert dyn._packed() is not p0 and torch.equal(dyn._packed()[2][5][2][1], dyn.ns_blocks[5].ln_1.offset.detach())
    pred, edyn = ez
    e0 = edyn._ez_packed(pred)
    assert edyn._ez_packed(pred) is e0
    pred.v_func.out.b.data = pred.v_func.out.b.data.clone()
    assert edyn._ez_packed(pred) is not e0


# ---- head arrays ----
def test_head_arrays_are_the_positional_lists(resnet):
    pred, dyn = resnet
    rf, vf, pf = dyn.r_func, pred.v_func, pred.pi_func
    r = nn_._head_arrays(rf, [(65, 64), (64, 64)], 64, 21)
    v = nn_._head_arrays(vf, [(64, 16), (16, 16)], 16, 21)
    p = nn_._head_arrays(pf, [(64, 16)], 16, 18)
    old_tower = [rf[0].w, rf[2].w, rf[5].w, rf[5].b, rf[7].w, rf[7].b,
                 vf[0].w, vf[2].w, vf[5].w, vf[5].b, vf[7].w, vf[7].b,
                 pf[0].w, pf[3].w, pf[3].b, pf[5].w, pf[5].b]
    assert len(_lib.MzsTowerArgs.HEAD_FIELDS) == len(r + v + p) == 17
    assert [t.data_ptr() for t in r + v + p] == [t.data_ptr() for t in old_tower]
    assert len(_lib.MzsRootTailArgs.HEAD_FIELDS) == len(v + p) == 11
    assert [t.data_ptr() for t in v + p] == [t.data_ptr() for t in old_tower[6:]]
    assert all(a is b for a, b in zip(r + v + p, old_tower))  # the parameters themselves, no copies


def _made_head(n_convs, hidden, out, with_bias=True):
    g = torch.Generator().manual_seed(5)
    seq = nn_._head(16, n_convs, hidden, out, g)
    if not with_bias:
        seq[2 * n_convs + 1] = nn_.LazyHkLinear(hidden, with_bias=False, generator=g)
    with torch.no_grad():
        seq(torch.rand(1, 6, 6, 64, generator=g))
    return seq


def test_head_arrays_refuse_other_heads():
    assert nn_._head_arrays(_made_head(1, 16, 18), [(64, 16)], 16, 18) is not None
    assert nn_._head_arrays(_made_head(1, 32, 18), [(64, 16)], 16, 18) is None  # hidden width
    assert nn_._head_arrays(_made_head(2, 16, 18), [(64, 16)], 16, 18) is None  # an extra conv
    assert nn_._head_arrays(_made_head(1, 16, 18, with_bias=False), [(64, 16)], 16, 18) is None  # no bias
    assert nn_._head_arrays(_made_head(1, 16, 18), [(64, 16)], 16, 21) is None  # output width
    assert nn_._head_arrays(nn_._head(16, 1, 16, 18, None), [(64, 16)], 16, 18) is None  # not built yet


# ---- weight keeper ----
def _trio_tensors():
    g = torch.Generator().manual_seed(6)
    return [torch.randn(3, 5, generator=g) for _ in _lib.MLP_WEIGHT_NAMES]


def test_mlp_weights_keeps_the_struct_until_a_tensor_moves():
    params = _trio_tensors()
    assert len(params) == 18
    k = _call.MlpWeights(params)
    w, keep = k.get()
    assert isinstance(w, _lib.MzsMlpWeights) and w.struct_size == _call.C.sizeof(_lib.MzsMlpWeights)
    assert [getattr(w, n) for n in _lib.MLP_WEIGHT_NAMES] == [t.data_ptr() for t in params]
    assert k.get()[0] is w
    params[3].add_(1)  # in place, as an optimiser writes: the struct stays
    assert k.get()[0] is w
    k.params[3] = k.params[3].clone()
    w2, keep2 = k.get()
    assert w2 is not w and w2.pv_b1 == k.params[3].data_ptr() and keep2[3].data_ptr() == w2.pv_b1
    assert k.get()[0] is w2


def test_mlp_weights_holds_a_contiguous_copy_of_a_strided_tensor_and_never_caches_it():
    params = _trio_tensors()
    params[2] = torch.randn(5, 3).t()  # [3, 5], strided
    k = _call.MlpWeights(params)
    w, keep = k.get()
    assert keep[2].is_contiguous() and torch.equal(keep[2], params[2]) and w.pv_w1 == keep[2].data_ptr() != params[2].data_ptr()
    assert [getattr(w, n) for n in _lib.MLP_WEIGHT_NAMES] == [t.data_ptr() for t in keep]
    w2, keep2 = k.get()
    assert w2 is not w and keep2[2] is not keep[2]  # a copy would go stale under an in-place update: made anew


# ---- helpers ----
def test_capture_holds_the_cyclic_collector_off_and_restores_it(monkeypatch):
    import contextlib
    import gc
    seen = []

    @contextlib.contextmanager
    def fake_graph(g):
        seen.append(("begin", g, gc.isenabled()))
        yield
        seen.append(("end", g, gc.isenabled()))
    monkeypatch.setattr(torch.cuda, "graph", fake_graph)
    assert gc.isenabled()
    with _call.capture("g"):
        assert not gc.isenabled()
    assert gc.isenabled() and seen == [("begin", "g", False), ("end", "g", False)]
    with pytest.raises(KeyError):  # an error under capture leaves through the graph's exit and restores the collector
        with _call.capture("g"):
            raise KeyError
    assert gc.isenabled() and len(seen) == 3  # (the fake never reaches its end after an error)
    gc.disable()
    try:
        with _call.capture("g"):
            pass
        assert not gc.isenabled()  # a caller that had it off keeps it off
    finally:
        gc.enable()


def test_device_index(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 5)
    assert _call.device_index(torch.device("cuda")) == 5
    assert _call.device_index(torch.device("cuda", 3)) == 3
