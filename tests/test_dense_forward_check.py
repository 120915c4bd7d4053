"""The fused Dense forwards' C++ checks and plans against their Python mirrors, on the CPU:
``csrc/tests/dense_fwd_check.cpp`` (a host program over ``sml_dense_fwd_plan.h``, ``sml_dense_fwdw_plan.h``
and ``sml_dense_fleet_fwd.h``) against ``ops/dense_forward.py``, ``ops/dense_forward_wide.py`` and
``ops/dense_fleet_forward.py``, word for word and number for number."""
import os
import subprocess

import pytest

import streamml
from streamml.ops import dense_fleet_forward as dff
from streamml.ops import dense_forward as dfw
from streamml.ops import dense_forward_wide as dfww
from test_dense_forward_limits import LIMITS as NARROW_LIMITS
from test_dense_forward_wide import LIMITS as WIDE_LIMITS

PKG = os.path.dirname(os.path.abspath(streamml.__file__))
FLEET = 6    # models of the fleet asked about

#        widths (input first), activation names, score
SHAPES = [([7, 7], ["tanh"], True), ([18, 33, 18], ["tanh", "linear"], True), ([128, 128], ["relu"], True),
          ([18, 512, 512, 512, 18], ["tanh", "relu", "tanh", "linear"], True), ([31, 31], ["sigmoid"], True),
          ([1, 1], ["linear"], False)]
# (name, widths, activation names, score, the limits table's words for the narrow kernel / for the wide one, or None)
CASES = ([(n, [feat] + widths, acts, score, words, None) for n, (widths, acts, feat, score, words) in NARROW_LIMITS.items()] +
         [("wide:" + n, [feat] + widths, acts, score, None, words) for n, (widths, acts, feat, score, words) in WIDE_LIMITS.items()] +
         [("-".join(map(str, w)), w, acts, score, None, None) for w, acts, score in SHAPES])


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")   # the host compiler the package itself is built with
    exe = str(tmp_path_factory.mktemp("dense_fwd_check") / "dense_fwd_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(PKG, "csrc", "include"),
                    os.path.join(PKG, "csrc", "tests", "dense_fwd_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=120)
    return exe


def _ask(checker, mode, n):
    """[(reason, [image units, plan numbers ...])] of every case, from one run of the host program."""
    text = "".join(f"{','.join(map(str, w))} {','.join(str(dfw.ACT.get(a, -1)) for a in acts)} {int(score)} {n}\n"
                   for _, w, acts, score, _, _ in CASES)
    r = subprocess.run([checker, mode], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [ln.split("\t") for ln in r.stdout.splitlines()]
    assert len(got) == len(CASES)
    return [(g[0], [int(v) for v in g[1:]]) for g in got]


def _layers(widths, acts):
    return [(i, o, a, True) for i, o, a in zip(widths[:-1], widths[1:], acts)]


def test_narrow_check_and_plan(checker):
    for (name, widths, acts, score, words, _), (why, nums) in zip(CASES, _ask(checker, "narrow", 0)):
        assert why == dfw.check_shape(widths, acts, score), name
        if words is not None:   # a row of the narrow limits table: the C++ side names that limit too
            assert (why == "") == (words == "") and words in why, (name, why)
        if not why:
            p = dfw.plan(widths)
            assert nums == [dfw.image_table(_layers(widths, acts))[1], p["mb"], p["stride"], p["waves"], p["lds_bytes"]], name


@pytest.mark.parametrize("rows", dfww.ROWS)
def test_wide_check_and_plan(checker, rows):
    for (name, widths, acts, score, _, words), (why, nums) in zip(CASES, _ask(checker, "wide", rows)):
        assert why == dfww.check_shape(widths, acts, score), name
        if words is not None:   # a row of the wide limits table
            assert (why == "") == (words == "") and words in why, (name, why)
        if not why:
            p = dfww.plan(widths, rows)
            assert nums == [dfww.image_table(_layers(widths, acts))[1], p["rows"], p["stride"], p["lds_bytes"]], name


def test_fleet_check_and_plan(checker):
    for (name, widths, acts, score, words, _), (why, nums) in zip(CASES, _ask(checker, "fleet", FLEET)):
        assert why == dff.check_shape(widths, acts, score, FLEET), name
        if words is not None:   # the fleet has the single-model kernel's limits
            assert (why == "") == (words == "") and words in why, (name, why)
        if not why:
            p = dff.plan(widths)
            assert nums == [dfw.image_table(_layers(widths, acts))[1]] + [p[k] for k in ("mb", "nbuf", "img2_off", "waves",
                                                                                          "stride", "lds_bytes")], name
    for n_models in (0, 1 << 24):
        for (name, widths, acts, score, _, _), (why, _) in zip(CASES, _ask(checker, "fleet", n_models)):
            assert why == dff.check_shape(widths, acts, score, n_models), name


def test_one_case_on_the_command_line(checker):
    r = subprocess.run([checker, "wide", "18,512,512,512,18", "2,1,2,0", "1", "128"], capture_output=True, text=True, timeout=60)
    p = dfww.plan([18, 512, 512, 512, 18], 128)
    assert r.returncode == 0 and r.stdout.split("\t")[0] == "" and [int(v) for v in r.stdout.split("\t")[2:]] == [
        128, p["stride"], p["lds_bytes"]]
    assert subprocess.run([checker, "other"], capture_output=True, timeout=60).returncode == 2


@pytest.mark.gpu
def test_bindings_refuse_the_same_arguments_in_the_same_words(cuda_device):
    """The three bindings check their tensors through one helper: the same bad arguments on the smallest
    stack (1-1, one row) are refused in the same words by each, before anything is launched."""
    import numpy as np
    import torch
    from streamml.ops import load_c
    C, dev = load_c(), cuda_device
    layers, weights = [(1, 1, "linear", True)], [(np.ones((1, 1), np.float32), np.zeros(1, np.float32))]
    img, table = dfw.pack_image(layers, weights)
    wimg, wtable = dfww.pack_image(layers, weights)
    img_d, wimg_d = torch.from_numpy(img).to(dev), torch.from_numpy(wimg.view(np.int16)).to(dev)
    imgs_d = torch.cat([img_d, torch.zeros(dff._img_pad(img.size) - img.size, device=dev)]).reshape(1, -1)
    table, wtable = [list(t) for t in table], [list(t) for t in wtable]
    rows, pair_base = torch.tensor([[0, 1]]), torch.tensor([0, 1])
    rows_d, pair_base_d = rows.to(dev), pair_base.to(dev)
    x, one = torch.zeros((1, 1), device=dev), lambda *s, **k: torch.zeros(s, device=dev, **k)

    def calls(scale=None, shift=None, rec=None, score=None, flag=None, sums=False, y=None, max_blocks=0):
        return [lambda: C.dense_forward(x, img_d, table, scale, shift, rec, score, flag, 0.0, sums, y, max_blocks),
                lambda: C.dense_forward_wide(x, wimg_d, wtable, scale, shift, rec, score, flag, 0.0, sums, y, max_blocks, 0),
                lambda: C.dense_forward_fleet(x, imgs_d, table, rows, rows_d, pair_base_d, scale, shift, rec, score, flag,
                                              one(1) if flag is not None else None, sums, y, max_blocks, False)]

    bad = [(dict(rec=one(2, 1)), ["rec must be a contiguous [n, 1]"] * 3),
           (dict(rec=one(1, 1), flag=one(1, dtype=torch.bool)), ["flags need scores"] * 2 + ["flags need scores and thresholds"]),
           (dict(score=one(1), sums=True, y=one(1, 1)), ["own targets are for sums alone"] * 3),
           (dict(rec=one(1, 1), scale=one(1)), ["scale and shift come together"] * 3),
           (dict(rec=one(1, 1), max_blocks=-1), ["bad max_blocks"] * 3)]
    for kwargs, words in bad:
        for call, want in zip(calls(**kwargs), words):
            with pytest.raises(RuntimeError) as e:
                call()
            assert str(e.value).splitlines()[0] == want, (sorted(kwargs), str(e.value)[:200])
