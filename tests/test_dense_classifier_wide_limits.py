"""The softmax head of the wide Dense kernels, checked without a device: which classifiers
``ops.dense_batch_wide.supports`` and ``ops.dense_forward_wide.supports(head=True)`` take, the word of the
reason for every combination they refuse, and what ``fit(engine="wide")`` says on the CPU."""
import numpy as np
import pytest

from streamml import nn
from streamml.nn.layers import L1L2, Dense
from streamml.ops import dense_batch_wide as dbw
from streamml.ops import dense_forward_wide as dfww

SCE = "sparse_categorical_crossentropy"


def _clf(widths, acts=None, loss=SCE, head_reg=None):
    acts = acts or ["tanh"] * (len(widths) - 2) + ["softmax"]
    layers = [Dense(u, a, input_shape=(widths[0],) if i == 0 else None,
                    activity_regularizer=head_reg if i == len(acts) - 1 else None)
              for i, (u, a) in enumerate(zip(widths[1:], acts))]
    model = nn.Sequential(layers, device="cpu", seed=13)
    model.compile(loss=loss)
    return model


# (model, own_targets, score) -> the word of the trainer's reason, of the forward's reason ("": accepted)
@pytest.mark.parametrize("make,own,score,train_word,fwd_word", [
    (lambda: _clf((18, 64, 2)), True, False, "", ""),
    (lambda: _clf((30, 512, 130)), True, False, "", ""),
    (lambda: _clf((512, 512, 512)), True, False, "", ""),
    (lambda: _clf((18, 64, 2), loss="mse"), True, False, "softmax under mean_squared_error", ""),
    (lambda: _clf((18, 64, 2), acts=["tanh", "linear"]), True, False, "needs a softmax head", "final softmax layer"),
    (lambda: _clf((18, 64, 18)), False, True, "needs labels", "scores need a reconstruction, not a softmax head"),
    (lambda: _clf((18, 64, 1)), True, False, "1 unit", "2..512 units"),
    (lambda: _clf((18, 64, 2), head_reg=L1L2(1e-3, 0.0)), True, False, "regularizer on the softmax head", ""),
    (lambda: _clf((18, 64, 8, 2), acts=["tanh", "softmax", "softmax"]), True, False, "softmax in the middle",
     "layer 1: unknown activation"),
    (lambda: _clf((18, 64, 2), loss="categorical_crossentropy"), True, False, "'categorical_crossentropy'", ""),
    (lambda: _clf((18, 64, 2), loss="binary_crossentropy"), True, False, "'binary_crossentropy'", ""),
], ids=["18-64-2", "30-512-130", "512-512-512", "mse", "linear_head", "y_is_x_and_score", "one_unit", "head_regulariser",
        "middle", "categorical", "binary"])
def test_supports_takes_classifiers_and_names_what_it_refuses(make, own, score, train_word, fwd_word):
    model = make()
    for (ok, why), word in ((dbw.supports(model, 256, own_targets=own), train_word),
                            (dfww.supports(model, score=score, head=True), fwd_word)):
        assert (ok, why) == (True, "") if not word else (not ok and word in why), why
    if model.layers[-1].activation == "softmax":   # without head=True the forward refuses softmax as it always did
        assert dfww.supports(model)[1].endswith("unknown activation")


def test_fit_engine_wide_of_a_classifier_on_the_cpu():
    x = np.random.default_rng(0).uniform(0, 1, (64, 18)).astype(np.float32)
    with pytest.raises(ValueError, match="ROCm"):
        _clf((18, 64, 2)).fit(x, np.zeros(64, np.int64), batch_size=32, epochs=1, verbose=0, engine="wide")
