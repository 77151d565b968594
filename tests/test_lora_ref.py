"""CPU: the float64 restatement of the LoRA kernels (tests/lora_ref.py) against the reference's formula written out with
F.linear in float64 -- the x path (LoRA.forward: q, k, v are row blocks 0, 1, 2 of in_proj, o is out_proj) and the v path
(LoRA.forward_qkv) -- and against float64 autograd of the unmerged form for dA and dB."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lora_ref as R

E, r, N, T, HEADS = 16, 3, 2, 5, 2


def _params(targets, seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    p = dict(win=rn(3 * E, E) / 4, bin=rn(3 * E) / 10, wout=rn(E, E) / 4, bout=rn(E) / 10)
    for t in targets:
        p["a_" + t], p["b_" + t] = rn(r, E) / 4, rn(E, r) / 2
    return p


def _merged(p, targets, s):
    win, _ = R.merge_ref(p["win"].numpy(), [(p["a_" + t].numpy(), p["b_" + t].numpy()) if t in targets else None
                                             for t in "qkv"], s)
    wout = R.merge_ref(p["wout"].numpy(), [(p["a_o"].numpy(), p["b_o"].numpy())], s)[0] if "o" in targets else p["wout"].numpy()
    return torch.from_numpy(win), torch.from_numpy(np.asarray(wout))


def _adapter(p, t, x, s):
    return F.linear(F.linear(x, p["a_" + t]), p["b_" + t]) * s


def _x_path(p, targets, s, x):
    """[N, T, E] tokens -> attention output with the adapters as side paths (the unmerged form)"""
    q, k, v = F.linear(x, p["win"], p["bin"]).chunk(3, dim=-1)
    q = q + _adapter(p, "q", x, s) if "q" in targets else q
    k = k + _adapter(p, "k", x, s) if "k" in targets else k
    v = v + _adapter(p, "v", x, s) if "v" in targets else v
    return _attend(q, k, v, p, targets, s)


def _attend(q, k, v, p, targets, s, wout=None):
    D = E // HEADS
    sp = lambda t: t.view(N, T, HEADS, D).transpose(1, 2)
    att = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / np.sqrt(D), dim=-1) @ sp(v)
    o = att.transpose(1, 2).reshape(N, T, E)
    if wout is not None:
        return F.linear(o, wout, p["bout"])
    out = F.linear(o, p["wout"], p["bout"])
    return out + _adapter(p, "o", o, s) if "o" in targets else out


def _v_path(p, targets, s, x):
    """the return_qkv blocks: every token's q | k | v through out_proj (and its adapter), unmerged"""
    qkv = F.linear(x, p["win"], p["bin"]).clone()
    for i, t in enumerate("qkv"):
        if t in targets:
            qkv[..., i * E:(i + 1) * E] += _adapter(p, t, x, s)
    qkv3 = qkv.view(N, T, 3, E).permute(2, 0, 1, 3).reshape(3 * N, T, E)
    out = F.linear(qkv3, p["wout"], p["bout"])
    return out + _adapter(p, "o", qkv3, s) if "o" in targets else out


@pytest.mark.parametrize("targets,s", [("qkvo", 2.0), ("qv", 0.5), ("o", 1.0), ("k", -1.5)])
def test_merged_weights_give_both_reference_forms(targets, s):
    p = _params(targets, seed=len(targets))
    x = torch.randn(N, T, E, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    win, wout = _merged(p, targets, s)
    q, k, v = F.linear(x, win, p["bin"]).chunk(3, dim=-1)
    got_x = _attend(q, k, v, p, targets, s, wout=wout)
    assert torch.allclose(got_x, _x_path(p, targets, s, x), rtol=0, atol=1e-12)
    qkv3 = F.linear(x, win, p["bin"]).view(N, T, 3, E).permute(2, 0, 1, 3).reshape(3 * N, T, E)
    got_v = F.linear(qkv3, wout, p["bout"])
    assert torch.allclose(got_v, _v_path(p, targets, s, x), rtol=0, atol=1e-12)
    for i, t in enumerate("qkv"):     # a block without a target is the base block, bit for bit
        if t not in targets:
            assert torch.equal(win[i * E:(i + 1) * E], p["win"][i * E:(i + 1) * E])


@pytest.mark.parametrize("s", [1.0, 2.5])
def test_projected_gradients_match_autograd(s):
    g = torch.Generator().manual_seed(3)
    rows, M = 24, 40
    x = torch.randn(M, E, generator=g, dtype=torch.float64)
    W = torch.randn(rows, E, generator=g, dtype=torch.float64)
    A = torch.randn(r, E, generator=g, dtype=torch.float64).requires_grad_()
    B = torch.randn(rows, r, generator=g, dtype=torch.float64).requires_grad_()
    G = torch.randn(M, rows, generator=g, dtype=torch.float64)
    (G * (F.linear(x, W) + s * F.linear(F.linear(x, A), B))).sum().backward()
    dW = (G.t() @ x).numpy()                 # the projection's full weight gradient
    dB, dA, magB, magA = R.wgrad_ref(dW, A.detach().numpy(), B.detach().numpy(), s)
    assert np.allclose(dA, A.grad.numpy(), rtol=0, atol=1e-11) and np.allclose(dB, B.grad.numpy(), rtol=0, atol=1e-11)
    assert (np.abs(dA) <= magA + 1e-12).all() and (np.abs(dB) <= magB + 1e-12).all()
    dB0, dA0 = np.ones((rows, r)), -np.ones((r, E))
    dB2, dA2, _, _ = R.wgrad_ref(dW, A.detach().numpy(), B.detach().numpy(), s, dB0, dA0)
    assert np.allclose(dB2, dB + 1.0, rtol=0, atol=1e-12) and np.allclose(dA2, dA - 1.0, rtol=0, atol=1e-12)


def test_gamma_is_highams():
    assert R.gamma(1) == pytest.approx(2.0 ** -24, rel=1e-6) and R.gamma(770) > 770 * 2.0 ** -24
