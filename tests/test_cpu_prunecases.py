"""What tests/test_gpu_chain_prune.py relies on, asserted from rdo_polyline and its taps alone (no GPU): every claim of every mask in tests/prunecases.py,
and the argument the prefilter rests on - a chain pixel whose 8-connected component has at most size_thre pixels ends with id 0."""
import numpy as np
import pytest

from tests import prunecases as pr

CASES = pr.all_cases()
BY = {c.name: c for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_claims(case):
    f = pr.facts(case)
    print(case.name, pr.resolve(case)[0].shape, f)
    for k, v in case.claims.items():
        assert f[k] == v, (case.name, k, f[k], v)
    ih, iw = pr.resolve(case)[0].shape
    assert iw <= 1100 and ih <= 400, case.name      # the planes stay small


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_small_components_end_with_id_0(case):
    """the prefilter's argument on the oracle's own output: no pixel of a component of at most size_thre pixels carries an id, and every live pixel is a survivor"""
    mask, _, (_, ids, info) = pr.resolve(case)
    pre, _ = pr.taps_run(mask, case.ring, case.minerror, case.size_thre)
    sizes = np.zeros(pre.shape, np.int64)
    sizes[pre] = pr.component_sizes(pre)
    got = ids.reshape(pre.shape) != 0
    assert not np.any(got & ~pre)
    assert not np.any(got & (sizes <= case.size_thre))
    assert info["live"] <= pr.facts(case)["survivors"]


def test_cases_say_what_they_mean():
    f = {n: pr.facts(c) for n, c in BY.items()}
    # the exact threshold: a component of exactly T pixels goes before the graph, one of T + 1 goes through it and the exact filter still drops it
    e = f["prefilter_edge_lines"]
    assert e["survivors"] < e["chain_pixels"] and e["live"] < e["survivors"]
    assert f["prefilter_edge_diamond_T11"]["survivors"] == 12 and f["prefilter_edge_diamond_T12"]["survivors"] == 0
    # the bench stream's shares: most chain pixels are dropped, and they mix with the others in every wave
    m = f["mixed_waves"]
    assert m["chain_pixels"] >= 600 and m["dead_share"] >= 0.8 and m["mixed_waves"]
    assert f["none_survive"]["chain_pixels"] > 600 and f["none_survive"]["survivors"] == 0
    assert f["all_survive"]["survivors"] == f["all_survive"]["chain_pixels"] == m["chain_pixels"]
    assert np.array_equal(pr.resolve(BY["all_survive"])[0], pr.resolve(BY["mixed_waves"])[0])
    # the numbering's reach: three rounds of 32 hops cover 33^3 pixels, the clamp is the result behind them
    b = f["beyond_reach"]
    assert b["max_num"] == 33 ** 3 and b["at_max_num"] >= 6000 and b["chains"] == 1
    assert f["hop_edges"]["chain_pixels"] < 8192 < f["hop_edges_two_blocks"]["survivors"]
