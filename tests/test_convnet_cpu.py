"""vface_amd/convnet.py on the CPU: the BatchNorm fold, the (tap, channel) window packing, the packed-weight table and the engine cache
of the parameter containers.  Nothing here launches a kernel."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from vface_amd import packing
from vface_amd.convnet import ConvNetEngine, EngineOwner, fold_bn


def _rand(g, *shape, dtype=torch.float64):
    return torch.randn(*shape, generator=g, dtype=dtype)


def _bn(g, c, dtype=torch.float64):
    """(gamma, beta, mean, var) of a BatchNorm with c channels."""
    return (torch.rand(c, generator=g, dtype=dtype) + 0.5, _rand(g, c, dtype=dtype), _rand(g, c, dtype=dtype),
            torch.rand(c, generator=g, dtype=dtype) + 0.1)


# ---- fold_bn ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_fold_bn_works_in_the_dtype_of_its_inputs(dtype):
    """No cast inside: fp32 in, fp32 out; fp64 in, fp64 out.  Without a bias the result is, bit for bit, the two-term form
    ``beta - mean * scale``; with one, ``(b - mean) * scale + beta``: the packed weights of both engines hang on these bits."""
    g = torch.Generator().manual_seed(3)
    w, b = _rand(g, 8, 5, 3, 3, dtype=dtype), _rand(g, 8, dtype=dtype)
    gamma, beta, mean, var = _bn(g, 8, dtype)
    scale = gamma / torch.sqrt(var + 1e-5)
    wf, bf = fold_bn(w, gamma, beta, mean, var)
    assert wf.dtype == dtype and bf.dtype == dtype
    assert torch.equal(wf, w * scale[:, None, None, None]) and torch.equal(bf, beta - mean * scale)
    wf2, bf2 = fold_bn(w, gamma, beta, mean, var, b=b)
    assert wf2.dtype == dtype and bf2.dtype == dtype
    assert torch.equal(wf2, wf) and torch.equal(bf2, (b - mean) * scale + beta)
    assert torch.equal(fold_bn(w, gamma, beta, mean, var, 1e-5, torch.zeros(8, dtype=dtype))[1], bf)      # b=None is b = 0


def test_fold_bn_with_a_bias_is_exact_in_fp64():
    g = torch.Generator().manual_seed(5)
    for cin, cout, k, stride in ((3, 8, 7, 2), (8, 16, 3, 1), (16, 8, 1, 2)):
        w, b = _rand(g, cout, cin, k, k), _rand(g, cout)
        gamma, beta, mean, var = _bn(g, cout)
        x = _rand(g, 2, cin, 9, 10)
        ref = F.batch_norm(F.conv2d(x, w, b, stride=stride, padding=k // 2), mean, var, gamma, beta, False, 0.0, 1e-5)
        wf, bf = fold_bn(w, gamma, beta, mean, var, b=b)
        assert (F.conv2d(x, wf, bf, stride=stride, padding=k // 2) - ref).abs().max() < 1e-12


# ---- pack_conv_im2col ------------------------------------------------------------------------------------------------------------
def _window_rows(x, kh, kw, stride, cp):
    """[1, C, H, W] -> [OH*OW, kh*kw*cp]: every output pixel's window in (tap, channel) order, 'same' zero padding, channels
    zero-padded to cp -- the matrix ``vface_im2col`` builds."""
    c = x.shape[1]
    cols = F.unfold(F.pad(x, (0, 0, 0, 0, 0, cp - c)), (kh, kw), padding=((kh - 1) // 2, (kw - 1) // 2), stride=stride)   # (channel, tap) rows
    return cols[0].reshape(cp, kh * kw, -1).permute(2, 1, 0).reshape(-1, kh * kw * cp)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin,cin_pad", [(3, 8), (324, 328), (16, None)])
@pytest.mark.parametrize("kh,kw", [(7, 7), (1, 5), (5, 1), (1, 1)])
def test_pack_conv_im2col_is_the_convolution(kh, kw, cin, cin_pad, stride):
    g = torch.Generator().manual_seed(kh * 100 + kw * 10 + cin + stride)
    cout, cp = 4, cin_pad or cin
    w, x = _rand(g, cout, cin, kh, kw), _rand(g, 1, cin, 6, 7)
    wp = packing.pack_conv_im2col(w, cin_pad)
    assert wp.shape == (cout, kh * kw * cp) and wp.dtype == w.dtype and wp.is_contiguous()
    assert not bool(wp.reshape(cout, kh * kw, cp)[..., cin:].any())                # the pad columns are exactly zero
    ref = F.conv2d(x, w, stride=stride, padding=((kh - 1) // 2, (kw - 1) // 2))[0].reshape(cout, -1).t()
    assert (_window_rows(x, kh, kw, stride, cp) @ wp.t() - ref).abs().max() < 1e-12


def test_pack_conv_im2col_is_not_pack_conv_window():
    """``pack_conv_window`` walks 64-channel chunks first: one chunk (Cin = 64) is still (tap, channel), from two chunks on it is
    another order, and a GEMM of the im2col matrix with it would be silently wrong."""
    g = torch.Generator().manual_seed(9)
    w64, w128 = _rand(g, 4, 64, 3, 3), _rand(g, 4, 128, 3, 3)
    assert torch.equal(packing.pack_conv_im2col(w64), packing.pack_conv_window(w64))
    a, b = packing.pack_conv_im2col(w128), packing.pack_conv_window(w128)
    assert a.shape == b.shape and not torch.equal(a, b)
    assert torch.equal(a.sort(dim=1).values, b.sort(dim=1).values)             # the same numbers, differently ordered
    x = _rand(g, 1, 128, 5, 6)
    ref = F.conv2d(x, w128, padding=1)[0].reshape(4, -1).t()
    rows = _window_rows(x, 3, 3, 1, 128)
    assert (rows @ a.t() - ref).abs().max() < 1e-12 and (rows @ b.t() - ref).abs().max() > 1.0


# ---- ConvNetEngine.add_conv ------------------------------------------------------------------------------------------------------
def _engine(dtype=torch.float16):
    eng = object.__new__(ConvNetEngine)          # without hip.load(): the table alone, on the CPU
    eng.dtype, eng.dev, eng.P = dtype, torch.device("cpu"), {}
    return eng


def _sd(g, dtype=torch.float64):
    sd = {"c3.weight": _rand(g, 6, 16, 3, 3, dtype=dtype), "c3.bias": _rand(g, 6, dtype=dtype),
          "c7.weight": _rand(g, 5, 3, 7, 7, dtype=dtype),
          "c1.weight": _rand(g, 6, 16, 1, 1, dtype=dtype)}
    sd.update(zip(("bn.weight", "bn.bias", "bn.running_mean", "bn.running_var"), _bn(g, 6, dtype)))
    return sd


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_add_conv_packs_pads_and_folds(dtype):
    eng, sd = _engine(dtype), _sd(torch.Generator().manual_seed(1))
    eng.add_conv(sd, "c3", "bn", cout_pad=8)
    p = eng.P["c3"]
    wf, bf = fold_bn(sd["c3.weight"], sd["bn.weight"], sd["bn.bias"], sd["bn.running_mean"], sd["bn.running_var"], b=sd["c3.bias"])
    assert (p["kind"], p["kh"], p["kw"], p["cin"], p["cout"]) == ("conv3", 3, 3, 16, 8)
    assert p["w"].dtype == dtype and p["w"].shape == (8, 144) and p["b"].dtype == torch.float32 and p["b"].shape == (8,)
    assert torch.equal(p["w"][:6], packing.pack_conv3x3(wf.float()).to(dtype)) and torch.equal(p["b"][:6], bf.float())
    assert not bool(p["w"][6:].any()) and not bool(p["b"][6:].any())              # pad rows and pad biases are exactly zero
    eng.add_conv(sd, "c7", cin_pad=8, cout_pad=8)
    p = eng.P["c7"]
    assert (p["kind"], p["kh"], p["kw"], p["cin"], p["cout"]) == ("gemm", 7, 7, 3, 8) and p["b"] is None
    assert torch.equal(p["w"][:5], packing.pack_conv_im2col(sd["c7.weight"].float(), 8).to(dtype)) and not bool(p["w"][5:].any())
    assert p["w"].shape == (8, 392) and p["w"].is_contiguous()


def test_add_conv_bias_is_none_only_without_a_bias_and_a_batchnorm():
    eng, sd = _engine(), _sd(torch.Generator().manual_seed(2), torch.float32)
    eng.add_conv(sd, "c1")
    eng.add_conv(sd, "c1", "bn", store="c1.bn")
    eng.add_conv(sd, "c3")
    eng.add_conv(sd, "c3", "bn", store="c3.bn")
    assert sorted(eng.P) == ["c1", "c1.bn", "c3", "c3.bn"]                       # store= renames the entry
    assert eng.P["c1"]["b"] is None
    assert torch.equal(eng.P["c3"]["b"], sd["c3.bias"])
    scale = sd["bn.weight"] / torch.sqrt(sd["bn.running_var"] + 1e-5)             # an fp32 state dict is folded in fp32
    assert torch.equal(eng.P["c1.bn"]["b"], sd["bn.bias"] - sd["bn.running_mean"] * scale)
    assert torch.equal(eng.P["c3.bn"]["b"], (sd["c3.bias"] - sd["bn.running_mean"]) * scale + sd["bn.bias"])
    assert all(eng.P[k]["b"].dtype == torch.float32 for k in ("c3", "c1.bn", "c3.bn"))


def test_add_conv_pooled_is_contiguous_fp32():
    eng, sd = _engine(torch.bfloat16), _sd(torch.Generator().manual_seed(4))
    eng.add_conv(sd, "c1", "bn", pooled=True)
    eng.add_conv(sd, "c1", pooled=True, store="plain")
    p, q = eng.P["c1"], eng.P["plain"]
    wf, bf = fold_bn(sd["c1.weight"], sd["bn.weight"], sd["bn.bias"], sd["bn.running_mean"], sd["bn.running_var"])
    assert p["w"].dtype == torch.float32 and p["w"].shape == (6, 16) and p["w"].is_contiguous() and (p["cout"], p["cin"]) == (6, 16)
    assert torch.equal(p["w"], wf.reshape(6, 16).float()) and torch.equal(p["b"], bf.float())
    assert q["b"] is None and torch.equal(q["w"], sd["c1.weight"].reshape(6, 16).float())


def test_both_engines_refuse_an_fp32_compute_type_at_construction():
    """Before any weight is packed or anything is launched."""
    from vface_amd import hip, parsing, raft
    with pytest.raises(hip.VFaceHipError, match="fp16 or bf16"):
        ConvNetEngine(torch.float32, "cpu")
    for cls in (raft.RaftEngine, parsing.ParseEngine):
        assert issubclass(cls, ConvNetEngine)
        with pytest.raises(hip.VFaceHipError, match="fp16 or bf16"):
            cls({}, torch.float32, "cpu")
    assert raft.RaftEngine.split_k is True and parsing.ParseEngine.split_k is False


# ---- EngineOwner -----------------------------------------------------------------------------------------------------------------
class _Owner(EngineOwner, nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(2, 2)
        self.made = 0

    def _make_engine(self):
        self.made += 1
        return ("engine", self.made)


def test_engine_owner_builds_once_and_drops_on_load_and_cast():
    m = _Owner()
    assert m._engine is None and m.made == 0
    assert m.engine is m.engine and m.made == 1
    m.load_state_dict(m.state_dict())
    assert m._engine is None and m.engine == ("engine", 2)
    assert m.to(torch.float64) is m and m._engine is None and m.engine == ("engine", 3)
    assert m.half() is m and m._engine is None and m.engine == ("engine", 4)
    assert m.lin.weight.dtype == torch.float16 and "_engine" not in m.state_dict()
