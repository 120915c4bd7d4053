"""float64 reference of the persistent Dense scorer (``csrc/kernels/dense_serve.hip``).

``forward`` runs a layer table (``ops.serve.dense_layer_table``) in float64; ``forward_image``
runs the same arithmetic from the packed weight image (``ops.serve.dense_serve_image``) instead
of the weights, so the layout can be checked without a device; ``relerr`` is the norm-relative
error the tests bound."""
import numpy as np

TILE = 32


def _act(name, z):
    if name in (None, "linear"):
        return z
    if name == "relu":
        return np.maximum(z, 0.0)
    if name == "tanh":
        return np.tanh(z)
    if name == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    raise ValueError(name)


def forward(layers, weights, xn):
    """y [k, D] (float64) of the stack over normalised rows xn [k, D]."""
    h = np.asarray(xn, np.float64)
    for (n_in, n_out, act, _), (W, b) in zip(layers, weights):
        z = h @ np.asarray(W, np.float64)
        if b is not None:
            z = z + np.asarray(b, np.float64)
        h = _act(act, z)
    return h


def unpack_image(image, table):
    """[(W [in, out], b [out], Wp [Kp, Np], bp [Np])] read back from the packed image: entry
    ``W[k][o]`` is float ``w_off + ((k // 4) * Np + o) * 4 + k % 4``, ``b[o]`` is ``b_off + o``."""
    out = []
    for n_in, n_out, _, w_off, b_off in table:
        kp, npad = (n_in + 3) // 4 * 4, (n_out + TILE - 1) // TILE * TILE
        Wp = np.empty((kp, npad), np.float32)
        for k in range(kp):
            Wp[k] = image[w_off + (k // 4) * npad * 4 + k % 4: w_off + (k // 4 + 1) * npad * 4: 4]
        bp = np.asarray(image[b_off:b_off + npad], np.float32)
        out.append((Wp[:n_in, :n_out].copy(), bp[:n_out].copy(), Wp, bp))
    return out


def forward_image(layers, image, table, xn):
    """``forward`` with weights and biases read from the packed image."""
    ws = [(W, b) for W, b, _, _ in unpack_image(image, table)]
    return forward(layers, ws, xn)


def score(y, xn):
    return np.mean((np.asarray(y, np.float64) - np.asarray(xn, np.float64)) ** 2, axis=1)


def relerr(got, want):
    """max over rows of |got - want| / |want| (2-norms)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.ndim == 1:
        got, want = got[:, None], want[:, None]
    return float(np.max(np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)))
