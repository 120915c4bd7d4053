"""Float64 forward of an ``LSTMPredictor`` stack over one window, for the per-event forecaster.

``forward(model, window)`` is the plain float64 oracle (Keras stateless semantics, gate order
i, f, c, o, sigmoid recurrent activation), as in tests/test_lstm_serve_gpu.py.

``forward(model, window, rounded=True)`` rounds to bf16 at exactly the points the wide kernel
does (the precision contract at the top of csrc/kernels/lstm_serve_wide.hip) and computes
everything else in float64:

* W and U of every LSTM layer;
* the normalised window x;
* h_t of every LSTM layer where it feeds the next step's recurrence and where it becomes the
  next layer's input sequence (also through a RepeatVector).

Biases, the gates, the cell state, the h that the Dense head reads and the head itself are
not rounded.
"""
import numpy as np
import torch

from .bf16_ref import bf


def stack_weights(model, rounded=False):
    """Per-layer float64 tensors of the model, rounded as forward(..., rounded) needs them
    (compute once per model, pass as ``weights``)."""
    P = [torch.as_tensor(np.asarray(a)).to(torch.float64) for a in model.fp.get()]
    out = []
    for L in model.layers:
        if L["kind"] == "lstm":
            W, U, b = P[L["params"]:L["params"] + 3]
            out.append((bf(W), bf(U), b) if rounded else (W, U, b))
        elif L["kind"] == "dense":
            out.append(tuple(P[L["params"]:L["params"] + 2]))
        else:
            out.append(())
    return out


def forward(model, window, rounded=False, weights=None):
    """[T, F] normalised window -> forecast [F]; [B, T, F] windows -> [B, F] (float64 numpy)."""
    weights = weights if weights is not None else stack_weights(model, rounded)
    rnd = bf if rounded else (lambda t: t)
    x = torch.as_tensor(np.asarray(window)).to(torch.float64)
    single = x.dim() == 2
    h = rnd(x[None] if single else x)   # the layer input, as the kernel holds it
    B = h.shape[0]
    last = None                         # unrounded h of the last LSTM step
    for L, P in zip(model.layers, weights):
        if L["kind"] == "lstm":
            W, U, b = P
            u = L["units"]
            hh = torch.zeros(B, u, dtype=torch.float64)
            c = torch.zeros(B, u, dtype=torch.float64)
            act = torch.relu if L["activation"] == "relu" else torch.tanh
            zx = h @ W + b
            outs = []
            for t in range(h.shape[1]):
                z = zx[:, t] + rnd(hh) @ U
                i, f, g, o = z.split(u, dim=1)
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * act(g)
                hh = torch.sigmoid(o) * act(c)
                outs.append(rnd(hh))
            last = hh
            h = torch.stack(outs, 1) if L["return_sequences"] else rnd(hh)
        elif L["kind"] == "repeat":
            h = h[:, None].expand(B, L["n"], h.shape[-1])
        else:
            K, b = P
            if rounded:   # the head reads the last LSTM step's h as computed, not its bf16 copy
                assert last is not None and L is model.layers[-1]
                h = last @ K + b
            else:
                h = h @ K + b
    out = (h[:, -1] if h.dim() == 3 else h).double().numpy()
    return out[0] if single else out


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12))
