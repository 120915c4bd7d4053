"""The fused MNIST-classifier train step's limits, checked without a device: ``ops.mlp_step.supports``
names the limit a model exceeds, and ``fit(engine="fused")`` says why it cannot run."""
import numpy as np
import pytest

from streamml.models.mlp import MLPClassifier
from streamml.ops import mlp_step


@pytest.mark.parametrize("batch,features,hidden,classes,world,word", [
    (33, 784, 128, 10, 1, "MLS_MAXBATCH"),
    (32, 1025, 128, 10, 1, "MLS_MAXIN"),
    (32, 784, 513, 10, 1, "MLS_MAXHIDDEN"),
    (32, 784, 128, 1, 1, "MLS_MAXCLASSES"),
    (32, 784, 128, 65, 1, "MLS_MAXCLASSES"),
    (32, 784, 128, 10, 2, "world size 2"),
], ids=["batch33", "in1025", "hidden513", "classes1", "classes65", "world2"])
def test_supports_names_the_limit(batch, features, hidden, classes, world, word):
    model = MLPClassifier(hidden=hidden, classes=classes, input_shape=(features,), device="cpu")
    ok, why = mlp_step.supports(model, batch, world=world)
    assert not ok and word in why, why


def test_fit_engine_fused_on_the_cpu():
    model = MLPClassifier(hidden=16, classes=4, input_shape=(6,), device="cpu")
    assert mlp_step.check(32, 6, 16, 4) == "" and mlp_step.check(1, 1024, 512, 64, 0.5) == ""
    x = np.random.default_rng(0).integers(0, 256, (40, 6), dtype=np.uint8)
    y = np.arange(40) % 4
    with pytest.raises(ValueError, match="not on a ROCm device"):
        model.fit(x, y, batch_size=32, verbose=0, engine="fused")
    with pytest.raises(ValueError, match="engine"):
        model.fit(x, y, batch_size=32, verbose=0, engine="fast")
    for engine in ("layers", "auto"):
        model.fit(x, y, batch_size=32, verbose=0, engine=engine)
        assert model.last_fit_engine == "layers"
