"""The fleet forward's host side without a device: ``ops.dense_fleet_forward``'s plan and check against
``sml_dense_fleet_fwd.h`` through the extension, the segment walk, and the thresholds ``fleet
--threshold-quantile`` writes into ``index.json``."""
import json

import numpy as np
import pytest
import torch

from streamml.ops import dense_fleet_forward as dff
from streamml.ops import dense_forward as dfw
from streamml.ops import load_c
from streamml.ops.serve import DenseFleetScoringServer
from test_dense_fleet_serve import _write_dir

#         widths, (nbuf, waves) of the plan, or the words of the refusal
STACKS = [
    ([18, 33, 18], (2, 8)),
    ([18, 64, 16, 64, 18], (2, 8)),
    ([30, 128, 32, 128, 30], (2, 4)),
    ([64, 128, 128, 64], (1, 2)),                   # about 130 KiB of image: one buffer, two waves
    ([128, 128, 128, 128], "bytes of LDS: the limit is 163840"),
]


@pytest.mark.parametrize("widths,want", STACKS, ids=["-".join(map(str, w)) for w, _ in STACKS])
def test_plan_and_check_mirror_the_header(widths, want):
    C = load_c()
    acts = ["tanh"] * (len(widths) - 1)
    table = [[i, o, dfw.ACT[a], 0, 0] for i, o, a in zip(widths[:-1], widths[1:], acts)]
    assert C.dense_fleet_fwd_check(table, True, 6) == dff.check_shape(widths, acts, True, 6)
    if isinstance(want, str):
        assert want in dff.check_shape(widths, acts, True, 6)
        return
    p = dff.plan(widths)
    assert (p["nbuf"], p["waves"]) == want
    assert [p[k] for k in ("mb", "nbuf", "img2_off", "waves", "stride", "lds_bytes")] == C.dense_fleet_fwd_plan(table)
    assert p["lds_bytes"] + 1024 <= dfw.LDS_BYTES and p["img2_off"] % dff.IMG_ALIGN == 0
    for n_models in (0, 1 << 24):
        why = C.dense_fleet_fwd_check(table, True, n_models)
        assert why == dff.check_shape(widths, acts, True, n_models) and "1..16777215" in why
    rows = torch.tensor([[0, 40], [30, 11]])
    assert "model 1: rows 30 .. 30 + 11 lie outside the 40 rows" in C.dense_fleet_fwd_check(table, True, 2, rows, 40)
    assert "stride" in C.dense_fleet_fwd_check(table, True, 2, rows, 41, 100)


@pytest.mark.parametrize("grid", [1, 3, 7, 40])
def test_walk_covers_every_pair_once(grid):
    """Models without rows are stepped over, a grid larger than G leaves workgroups idle, and no two
    segments share a slot."""
    rows = np.array([0, 1, 0, 0, 33, 64, 0, 203, 17, 0])
    table = torch.from_numpy(np.stack([np.cumsum(rows) - rows, rows], axis=1).astype(np.int64))
    pair_base, segs = load_c().dense_fleet_fwd_walk(table, grid)
    pairs = -(-rows // dff.PAIR_ROWS)
    assert pair_base == [0] + np.cumsum(pairs).tolist()
    seen = [np.zeros(p, int) for p in pairs]
    for b, m, slot, p0, p1 in segs:
        assert 0 <= p0 < p1 <= pairs[m] and slot == m + b < len(rows) + grid
        seen[m][p0:p1] += 1
    assert all((s == 1).all() for s in seen)
    assert len({s[2] for s in segs}) == len(segs) <= (pairs > 0).sum() + grid - 1
    assert segs == sorted(segs) and len({s[0] for s in segs}) == min(grid, pairs.sum())


def test_index_thresholds(tmp_path):
    from streamml.cli.fleet import build_index
    members, names = [["car-a"], ["car-b"]], ["car-a", "car-b"]
    plain = build_index(names, members, [0.1, 0.2], (16,), "fp32")
    with_thr = build_index(names, members, [0.1, 0.2], (16,), "fp32", thresholds=np.array([0.5, 0.25], np.float32))
    assert json.dumps(plain, indent=1) == json.dumps(build_index(names, members, [0.1, 0.2], (16,), "fp32", None), indent=1)
    assert all("threshold" not in plain[n] for n in names)
    assert [with_thr[n].pop("threshold") for n in names] == [0.5, 0.25] and with_thr == plain
    _write_dir(str(tmp_path / "fleet"), members)
    with pytest.raises(ValueError, match="no 'threshold' for 'car-a'"):
        DenseFleetScoringServer.from_dir(str(tmp_path / "fleet"), thresholds="index", device="cpu")
