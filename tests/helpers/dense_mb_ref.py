"""float64 numpy reference of the Keras train step of an arbitrary Dense stack.

Forward, MSE + l1 / l2 activity penalties over the batch, categorical accuracy, backward and
Adam (epsilon outside the root), written out by hand: independent of torch autograd and of
the code under test.
"""
import numpy as np


def act_fwd(name, z):
    if name == "relu":
        return np.maximum(z, 0.0)
    if name == "tanh":
        return np.tanh(z)
    if name == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    assert name == "linear", name
    return z


def act_grad(name, h):
    """d act / dz through the activation output h."""
    if name == "relu":
        return (h > 0).astype(np.float64)
    if name == "tanh":
        return 1.0 - h * h
    if name == "sigmoid":
        return h * (1.0 - h)
    return np.ones_like(h)


class Layer:
    def __init__(self, W, b, activation="linear", l1=0.0, l2=0.0):
        self.W = np.asarray(W, np.float64).copy()
        self.b = None if b is None else np.asarray(b, np.float64).copy()
        self.activation, self.l1, self.l2 = activation, float(l1), float(l2)


class DenseRef:
    """``layers``: list of Layer; the Adam state is kept per array."""

    def __init__(self, layers, lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, iterations=0):
        self.layers = layers
        self.lr, self.b1, self.b2, self.eps = lr, beta_1, beta_2, epsilon
        self.t = int(iterations)
        self.m = [[np.zeros_like(L.W), None if L.b is None else np.zeros_like(L.b)] for L in layers]
        self.v = [[np.zeros_like(L.W), None if L.b is None else np.zeros_like(L.b)] for L in layers]
        self.min_top2_gap = np.inf   # over all rows seen: top-two gap of the outputs and of the targets
        self.pred_classes = set()    # every predicted class (argmax of an output row) seen
        self.max_classes_in_step = 0   # most distinct predicted classes within one step

    def forward(self, x):
        hs = [np.asarray(x, np.float64)]
        for L in self.layers:
            z = hs[-1] @ L.W
            if L.b is not None:
                z = z + L.b
            hs.append(act_fwd(L.activation, z))
        return hs

    def step(self, x, y=None):
        """One Keras step on the batch; returns (loss incl. penalties, rows with matching argmax)."""
        x = np.asarray(x, np.float64)
        y = x if y is None else np.asarray(y, np.float64)
        B = x.shape[0]
        hs = self.forward(x)
        yp = hs[-1]
        loss = np.mean((yp - y) ** 2)
        for L, h in zip(self.layers, hs[1:]):
            loss += (L.l1 * np.abs(h).sum() + L.l2 * (h * h).sum()) / B
        pred = yp.argmax(-1)
        correct = int((pred == y.argmax(-1)).sum())
        self.pred_classes.update(int(c) for c in pred)
        self.max_classes_in_step = max(self.max_classes_in_step, len(set(pred.tolist())))
        if yp.shape[1] > 1:
            for a in (yp, y):
                s = np.sort(a, axis=-1)
                self.min_top2_gap = min(self.min_top2_gap, float((s[:, -1] - s[:, -2]).min()))
        # backward
        g = 2.0 * (yp - y) / yp.size
        grads = [None] * len(self.layers)
        for i in range(len(self.layers) - 1, -1, -1):
            L, h = self.layers[i], hs[i + 1]
            g = g + (L.l1 * np.sign(h) + 2.0 * L.l2 * h) / B
            dz = g * act_grad(L.activation, h)
            grads[i] = (hs[i].T @ dz, dz.sum(0))
            g = dz @ L.W.T
        # Adam (tf.keras: lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t); p -= lr_t * m / (sqrt(v) + eps))
        self.t += 1
        lr_t = self.lr * np.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)
        for i, L in enumerate(self.layers):
            for k, (p, gk) in enumerate(((L.W, grads[i][0]), (L.b, grads[i][1]))):
                if p is None:
                    continue
                self.m[i][k] = self.b1 * self.m[i][k] + (1.0 - self.b1) * gk
                self.v[i][k] = self.b2 * self.v[i][k] + (1.0 - self.b2) * gk * gk
                p -= lr_t * self.m[i][k] / (np.sqrt(self.v[i][k]) + self.eps)
        return float(loss), correct

    def run(self, x, y, batch, nsteps, row0=0, order=None):
        """The steps ``train_steps`` runs: rows order[row0 + s * batch ...]; returns [nsteps, 2]."""
        n = len(x)
        out = []
        for s in range(nsteps):
            lo = row0 + s * batch
            if lo >= n:
                break
            idx = np.arange(lo, min(lo + batch, n))
            if order is not None:
                idx = np.asarray(order)[idx]
            out.append(self.step(x[idx], None if y is None else y[idx]))
        return np.asarray(out, np.float64)

    def weights(self):
        out = []
        for L in self.layers:
            out.append(L.W)
            if L.b is not None:
                out.append(L.b)
        return out

    def moments(self, which="m"):
        src = self.m if which == "m" else self.v
        return [a for pair in src for a in pair if a is not None]
