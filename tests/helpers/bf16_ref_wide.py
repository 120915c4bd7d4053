"""Float64 torch reference for the unfused LSTM path (``ops.lstm.LSTMFunction``: projection
GEMM + ``lstm_fwd`` / ``lstm_bwd`` recurrence kernels + weight-gradient GEMMs) that rounds to
bf16 exactly where that path does, in the pattern of ``bf16_ref.py``:

* x and W in the projection GEMM (zx itself, the bias, h, c and the gates stay fp32);
* U and h_{t-1} in the recurrence MFMAs;
* dz and U in the dh recurrence (dz is written out in fp32; dh_in is read in fp32);
* both operands of the dW = x^T.dz, dU = h_{t-1}^T.dz and dX = dz.W^T GEMMs; db sums fp32 dz.

What remains between kernel and reference is accumulation order, fp32 storage and the
hardware exp / rcp approximations.
"""
import torch

from .bf16_ref import _act, _act_d, bf, relerr  # noqa: F401  (relerr re-exported for the tests)


def lstm_recurrence_bf16_reference(zx, U, act="relu", h0=None, c0=None, dh=None):
    """``lstm_fwd`` (+ ``lstm_bwd`` when ``dh`` is given) on zx = x.W + b [B, T, 4u].

    Returns (h, c, gates) or (h, c, gates, dz, dh0, dc0), float64; gates are post-activation
    i | f | c~ | o as the kernel saves them."""
    zx = zx.double()
    B, T, _ = zx.shape
    u = U.shape[0]
    Ub = bf(U)
    h = torch.zeros(B, u, dtype=torch.float64) if h0 is None else h0.double()
    c = torch.zeros(B, u, dtype=torch.float64) if c0 is None else c0.double()
    c_init = c
    hs, cs, gs = [], [], []
    for t in range(T):
        z = zx[:, t] + bf(h) @ Ub
        zi, zf, zg, zo = z.split(u, dim=1)
        gi, gf, go = torch.sigmoid(zi), torch.sigmoid(zf), torch.sigmoid(zo)
        gc = _act(act, zg)
        c = gf * c + gi * gc
        h = go * _act(act, c)
        hs.append(h)
        cs.append(c)
        gs.append(torch.cat([gi, gf, gc, go], 1))
    hseq, cseq, gates = torch.stack(hs, 1), torch.stack(cs, 1), torch.stack(gs, 1)
    if dh is None:
        return hseq, cseq, gates
    dh = dh.double()
    dhr = torch.zeros(B, u, dtype=torch.float64)
    dcn = torch.zeros(B, u, dtype=torch.float64)
    dzs = [None] * T
    for t in range(T - 1, -1, -1):
        gi, gf, gc, go = gs[t].split(u, dim=1)
        ct = cs[t]
        cp = cs[t - 1] if t > 0 else c_init
        dht = dh[:, t] + dhr
        ac = _act(act, ct)
        dc = dcn + dht * go * _act_d(act, ct, ac)
        # the kernel takes the candidate's derivative from its saved output: relu'(z) = [relu(z) > 0]
        dz = torch.cat([dc * gc * gi * (1 - gi), dc * cp * gf * (1 - gf), dc * gi * _act_d(act, gc, gc),
                        dht * ac * go * (1 - go)], 1)
        dcn = dc * gf
        dzs[t] = dz
        dhr = bf(dz) @ Ub.t()
    return hseq, cseq, gates, torch.stack(dzs, 1), dhr, dcn


def lstm_unfused_bf16_reference(x, W, U, b, act="relu", dh=None):
    """The whole layer from zero state.  Returns h [B, T, u], or (h, dx, dW, dU, db)."""
    B, T, inp = x.shape
    u = U.shape[0]
    xb, Wb = bf(x), bf(W)
    zx = xb @ Wb + b.double()
    if dh is None:
        return lstm_recurrence_bf16_reference(zx, U, act)[0]
    h, _, _, dz, _, _ = lstm_recurrence_bf16_reference(zx, U, act, dh=dh)
    dzb = bf(dz).reshape(B * T, 4 * u)
    hprev = torch.cat([torch.zeros(B, 1, u, dtype=torch.float64), h[:, :-1]], 1)
    dW = xb.reshape(B * T, inp).t() @ dzb
    dU = bf(hprev).reshape(B * T, u).t() @ dzb
    db = dz.reshape(B * T, 4 * u).sum(0)
    dx = (dzb @ Wb.t()).reshape(B, T, inp)
    return h, dx, dW, dU, db
