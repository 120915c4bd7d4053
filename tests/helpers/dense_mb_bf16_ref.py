"""float64 oracle of ONE Keras step of the bf16 persistent Dense trainer
(csrc/kernels/dense_minibatch_bf16.hip), written out by hand like helpers/dense_mb_ref.DenseRef.

Rounding points (``bf`` = round to nearest even bf16), exactly those of the kernel's header:

* forward    z_l = b_l + bf(h_{l-1}) @ bf(W_l),  h_l = act(z_l) unrounded, h_0 = x;
* the unrounded h_l feeds the loss, the l1 / l2 penalties, the accuracy and the derivative;
* backward   g_{l-1} = bf(dz_l) @ bf(W_l)^T,  dz_{l-1} = act'(h_{l-1}) (g_{l-1} + penalty gradient);
* weights    dW_l = bf(h_{l-1})^T @ bf(dz_l);
* bias       db_l = column sum of the UNROUNDED dz_l (``db_bf16 = False``, the switch
  helpers/bf16_ref.py has for the LSTM kernels: the kernel sums fp32 dz, not bf(dz));
* Adam on the unrounded masters (helpers/dense_mb_ref's formulas).

``grads(..., kind="O")`` is that oracle.  ``kind="exact"`` is the same step with no rounding at
all.  ``kind="V"`` is a second legal evaluation of the same rounding points that models the
device's arithmetic: contractions accumulate in float32, K split in halves with the second half
first, every intermediate rounded to fp32, tanh / sigmoid outputs perturbed by uniform noise of
+-2.4e-7 (two fp32 ulps at 1.0: the error of tanh_fast / sigmoid_fast) before rounding.

A free-running comparison over a case's 24 steps is ill-conditioned (one flipped bf16 rounding or
relu gate compounds through Adam), so the GPU test compares ONE step at a time from the kernel's
own state, and pins the multi-step behaviour by bit-identity.

TOL_G, the bound on ||g_kernel - g_O|| / ||g_O|| over the whole flat gradient of a step, is
2 x the largest spread V shows against O (five seeds, steps {0, 1, 11, last} of every case, along
O's own trajectory); the factor 2 is there because V only models the device's rounding.  It must
stay below half the smallest gap ||g_exact - g_O|| / ||g_O|| (median over a case's steps) of the
four wide cases, or the bound could not tell the bf16 step from the fp32 one.
``measure()`` computes both; tests/test_dense_minibatch_bf16_gpu.py::test_tol_g_is_the_measured_one
recomputes them and asserts the constants pinned here.

Measured with ``measure()`` on the CPU (numpy float64 / float32, 17 cases):

    quantity                                                         measured
    spread ||g_V - g_O|| / ||g_O||, checked steps, largest           4.36e-4  (30-128-32-128-30_b32)
    same, the other wide cases                                       0.9e-4 .. 2.6e-4
    loss of V against O, largest relative difference                 3.0e-5
    ``correct`` of V against O                                       never differs
    gap ||g_exact - g_O|| / ||g_O||, median over the case's steps:
        18-64-16-64-18          7.80e-3
        30-128-32-128-30_b32    1.73e-2
        30-128-32-128-30_b100   1.27e-2
        eight_layers            8.18e-3
        one_layer               1.17e-3   (narrow: a tolerance alone cannot tell bf16 from fp32 there)

    TOL_G = 2 x 4.355e-4 = 8.71e-4  <=  half the smallest wide gap = 3.90e-3
"""
import numpy as np

from helpers.dense_mb_ref import act_fwd, act_grad

CHECKED = (0, 1, 11, -1)              # steps of a case the per-step checks look at
WIDE = ("18-64-16-64-18", "30-128-32-128-30_b32", "30-128-32-128-30_b100", "eight_layers")
V_SEEDS = (0, 1, 2, 3, 4)
NOISE = 2.4e-7

# ---- pinned by measure() (see the module docstring and test_tol_g_is_the_measured_one) ----
SPREAD_MAX = 4.355e-4
SPREAD_CASE = "30-128-32-128-30_b32"
GAP_MEDIANS = {"18-64-16-64-18": 7.80e-3, "30-128-32-128-30_b32": 1.73e-2, "30-128-32-128-30_b100": 1.27e-2,
               "eight_layers": 8.18e-3}
TOL_G = 2.0 * SPREAD_MAX


def bf(a):
    """Round to the nearest bf16 (ties to even), through fp32 as the device does; float64 out."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    u = (u + (((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64)


def _mm64(a, b):
    return a @ b


def _mm32_halves(a, b):
    """float32 accumulation, one rounding per multiply-add, the second half of K first."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    K = a.shape[1]
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for k in list(range(K // 2, K)) + list(range(K // 2)):
        acc = acc + a[:, k:k + 1] * b[k:k + 1, :]
    assert acc.dtype == np.float32
    return acc.astype(np.float64)


class Spec:
    """The stack: widths, activations and per layer bias / l1 / l2, as in dense_mb_cases.CASES."""

    def __init__(self, widths, acts, bias=None, l1=None, l2=None):
        nl = len(widths) - 1
        self.widths, self.acts = list(widths), list(acts)
        self.bias = list(bias) if bias is not None else [True] * nl
        self.l1 = list(l1) if l1 is not None else [0.0] * nl
        self.l2 = list(l2) if l2 is not None else [0.0] * nl
        self.nl = nl

    def shapes(self):
        out = []
        for l in range(self.nl):
            out.append((self.widths[l], self.widths[l + 1]))
            if self.bias[l]:
                out.append((self.widths[l + 1],))
        return out

    def split(self, flat):
        """The arrays (FlatParams order: kernel, bias, kernel, ...) of a flat vector, float64."""
        out, off = [], 0
        for s in self.shapes():
            n = int(np.prod(s))
            out.append(np.asarray(flat[off:off + n], np.float64).reshape(s))
            off += n
        return out

    def nparams(self):
        return sum(int(np.prod(s)) for s in self.shapes())


def flat_of(arrs):
    return np.concatenate([np.asarray(a, np.float64).ravel() for a in arrs])


def grads(spec, ws, x, y=None, kind="O", seed=0):
    """One step's (loss incl. penalties, rows with matching argmax, gradients in the order of ws)
    at the weights ``ws``.  kind: "O" the oracle, "exact" no rounding, "V" the device model."""
    assert kind in ("O", "exact", "V")
    rb = (lambda a: np.asarray(a, np.float64)) if kind == "exact" else bf
    mm = _mm32_halves if kind == "V" else _mm64
    r32 = (lambda a: np.asarray(a, np.float32).astype(np.float64)) if kind == "V" else (lambda a: a)
    rng = np.random.default_rng([seed, 77]) if kind == "V" else None
    ws = [np.asarray(w, np.float64) for w in ws]
    Ws, bs, k = [], [], 0
    for l in range(spec.nl):
        Ws.append(ws[k])
        k += 1
        bs.append(ws[k] if spec.bias[l] else None)
        k += 1 if spec.bias[l] else 0
    x = np.asarray(x, np.float64)
    y = x if y is None else np.asarray(y, np.float64)
    B = x.shape[0]
    hs = [x]
    for l in range(spec.nl):
        z = mm(rb(hs[-1]), rb(Ws[l]))
        if bs[l] is not None:
            z = r32(z + bs[l])
        h = act_fwd(spec.acts[l], z)
        if kind == "V" and spec.acts[l] in ("tanh", "sigmoid"):
            h = h + rng.uniform(-NOISE, NOISE, size=h.shape)
        hs.append(r32(h))
    yp = hs[-1]
    loss = np.mean((yp - y) ** 2)
    for l in range(spec.nl):
        h = hs[l + 1]
        loss += (spec.l1[l] * np.abs(h).sum() + spec.l2[l] * (h * h).sum()) / B
    correct = int((yp.argmax(-1) == y.argmax(-1)).sum())
    g = r32(2.0 * (yp - y) / yp.size)
    out = [None] * spec.nl
    for l in range(spec.nl - 1, -1, -1):
        h = hs[l + 1]
        g = r32(g + (spec.l1[l] * np.sign(h) + 2.0 * spec.l2[l] * h) / B)
        dz = r32(g * act_grad(spec.acts[l], h))
        dW = mm(rb(hs[l]).T, rb(dz))
        db = r32(dz.sum(0))
        out[l] = (dW, db)
        if l > 0:
            g = mm(rb(dz), rb(Ws[l]).T)
    gl = []
    for l in range(spec.nl):
        gl.append(out[l][0])
        if spec.bias[l]:
            gl.append(out[l][1])
    return float(loss), correct, gl


class Adam64:
    """float64 Keras Adam on a list of arrays (dense_mb_ref's update)."""

    def __init__(self, ws, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
        self.ws = [np.asarray(w, np.float64).copy() for w in ws]
        self.m = [np.zeros_like(w) for w in self.ws]
        self.v = [np.zeros_like(w) for w in self.ws]
        self.t, self.lr, self.b1, self.b2, self.eps = 0, lr, b1, b2, eps

    def apply(self, gl):
        self.t += 1
        lr_t = self.lr * np.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)
        for i, g in enumerate(gl):
            self.m[i] = self.b1 * self.m[i] + (1.0 - self.b1) * g
            self.v[i] = self.b2 * self.v[i] + (1.0 - self.b2) * g * g
            self.ws[i] = self.ws[i] - lr_t * self.m[i] / (np.sqrt(self.v[i]) + self.eps)


def relerr(a, b):
    """||a - b|| / ||b|| over whole flat gradients."""
    a, b = flat_of(a), flat_of(b)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def batches(x, y, order, batch):
    n = len(x)
    for s in range(-(-n // batch)):
        idx = np.arange(s * batch, min((s + 1) * batch, n))
        if order is not None:
            idx = np.asarray(order)[idx]
        yield s, x[idx], (None if y is None else y[idx])


def checked_steps(nsteps):
    return sorted({c % nsteps for c in CHECKED})


def measure_case(spec, ws, x, y, order, batch):
    """Along O's own trajectory: (largest ||g_V - g_O|| / ||g_O|| over V_SEEDS and the checked steps,
    median over ALL steps of ||g_exact - g_O|| / ||g_O||, largest relative loss difference of V,
    whether a ``correct`` count of V ever differed)."""
    opt = Adam64(ws)
    nsteps = -(-len(x) // batch)
    chk = checked_steps(nsteps)
    spread, gaps, dloss, dcorr = 0.0, [], 0.0, False
    for s, xb, yb in batches(x, y, order, batch):
        lo, co, go = grads(spec, opt.ws, xb, yb, "O")
        gaps.append(relerr(grads(spec, opt.ws, xb, yb, "exact")[2], go))
        if s in chk:
            for seed in V_SEEDS:
                lv, cv, gv = grads(spec, opt.ws, xb, yb, "V", seed)
                spread = max(spread, relerr(gv, go))
                dloss = max(dloss, abs(lv - lo) / abs(lo))
                dcorr = dcorr or cv != co
        opt.apply(go)
    return spread, float(np.median(gaps)), dloss, dcorr


def measure(names=None):
    """{case: (spread, gap median, loss spread, correct differed)} for the cases of
    helpers/dense_mb_bf16_cases (all of them by default)."""
    from helpers import dense_mb_bf16_cases as bcases
    out = {}
    for name in names or bcases.NAMES:
        ws, x, y, order = bcases.arrays(name)
        out[name] = measure_case(bcases.spec(name), ws, x, y, order, bcases.batch_of(name))
    return out
