"""CPU: the hubness summary (RetrievalMetrics.hubness_from_occurrences) on hand-worked k-occurrence counts, the NumPy
restatement it is checked against on the GPU (hubness_ref), and the host-side refusals of the top-k entry points."""
import ctypes

import numpy as np
import pytest

import hubness_ref as H
from neighborretr_amd import hip
from neighborretr_amd.metrics import RetrievalMetrics

hub_of = RetrievalMetrics.hubness_from_occurrences


def test_uniform_occurrences_have_no_skew_and_no_hubs():
    h = hub_of([3, 3, 3, 3], [1, 1, 1, 1], k=3, n_queries=4)
    assert h["mu"] == 3.0 and h["skewness"] == 0.0
    assert h["hub_pct"] == 0.0 and h["anti_hub_pct"] == 0.0 and h["bad_hub_pct"] == 0.0 and h["hub_occurrence_pct"] == 0.0
    assert h["good_occurrence_pct"] == 100.0 * 4 / 12
    assert h["max_occurrence"] == 3 and h["k"] == 3 and h["n_queries"] == 4 and h["n_gallery"] == 4
    assert h["occurrence"].dtype == np.int64 and h["good_occurrence"].dtype == np.int64


def test_one_dominant_hub():
    # 5 queries, k = 2: item 0 sits in every list, the second slots spread as N_k = [5, 2, 2, 1, 0]; mu = 2, hubs: N_k > 4 ->
    # item 0 only
    occ, good = [5, 2, 2, 1, 0], [1, 1, 0, 1, 0]
    h = hub_of(occ, good, k=2, n_queries=5)
    assert h["mu"] == 2.0
    assert h["hub_pct"] == 100.0 * 1 / 5
    assert h["hub_occurrence_pct"] == 100.0 * 5 / 10
    assert h["bad_hub_pct"] == 100.0 * 1 / 5                 # BN = 4 > GN = 1
    assert h["anti_hub_pct"] == 100.0 * 1 / 5
    assert h["good_occurrence_pct"] == 100.0 * 3 / 10
    assert h["max_occurrence"] == 5
    d = np.array(occ, dtype=np.float64) - 2.0                  # [3, 0, 0, -1, -2]: mean d^2 = 14/5, mean d^3 = 18/5
    assert h["skewness"] == pytest.approx((18 / 5) / (14 / 5) ** 1.5, rel=1e-12)
    assert h["skewness"] > 0


def test_all_anti_hubs_but_one():
    # every query retrieves the same single item (k = 1, 6 queries, 6 items): the extreme hub
    occ, good = [0, 0, 6, 0, 0, 0], [0, 0, 1, 0, 0, 0]
    h = hub_of(occ, good, k=1, n_queries=6)
    assert h["mu"] == 1.0
    assert h["anti_hub_pct"] == 100.0 * 5 / 6
    assert h["hub_pct"] == 100.0 * 1 / 6 and h["hub_occurrence_pct"] == 100.0
    assert h["bad_hub_pct"] == 100.0 * 1 / 6 and h["good_occurrence_pct"] == 100.0 / 6
    # mu = 1: d = [-1 x5, 5]; mean d^2 = 30/6 = 5, mean d^3 = (-5 + 125)/6 = 20
    assert h["skewness"] == pytest.approx(20 / 5 ** 1.5, rel=1e-12)


def test_multi_sentence_counts_through_the_reference_definitions():
    # 6 sentences, 3 videos: sentences {0, 1} describe video 0, {2, 3, 4} video 1, {5} video 2
    cut = [1, 4, 5]
    S = np.array([[0.9, 0.1, 0.2],
                  [0.3, 0.8, 0.1],
                  [0.2, 0.7, 0.6],
                  [0.5, 0.6, 0.4],
                  [0.1, 0.2, 0.3],
                  [0.4, 0.3, 0.9]], dtype=np.float32)
    t2v, v2t = H.hubness(S, 2, cut)
    # t2v (sentence -> 2 videos): lists {0,2} {1,0} {1,2} {1,0} {2,1} {2,0}
    assert t2v["occ"].tolist() == [4, 4, 4]
    # good: sentence s's video g(s) in its list: s0 (g0) yes, s1 (g0) yes, s2 (g1) yes, s3 (g1) yes, s4 (g1) yes, s5 (g2) yes
    assert t2v["good"].tolist() == [2, 3, 1]
    # v2t (video -> 2 sentences): v0 {0,3}, v1 {1,2}, v2 {5,2}
    assert v2t["occ"].tolist() == [1, 1, 2, 1, 0, 1]
    # good: v0's sentences {0,1}: 0; v1's {2,3,4}: 2; v2's {5}: 5
    assert v2t["good"].tolist() == [1, 0, 1, 0, 0, 1]
    h = hub_of(v2t["occ"], v2t["good"], k=2, n_queries=3)
    ref = H.summary(v2t["occ"], v2t["good"])
    for key, want in ref.items():
        assert h[key] == pytest.approx(want, rel=1e-12, abs=0), key
    assert h["n_gallery"] == 6 and h["anti_hub_pct"] == 100.0 / 6
    assert h["hub_pct"] == 0.0                                 # mu = 1: N_k = 2 is not above 2 mu


def test_reference_lists_follow_the_order_rules():
    S = np.array([[1.0, np.nan, -0.0, 0.0, np.inf, -np.inf, 1.0]], dtype=np.float32)
    idx, val = H.topk_lists(S, 7)
    assert idx.tolist() == [[4, 0, 6, 2, 3, 5, -1]]
    assert np.signbit(val[0, 3]) and not np.signbit(val[0, 4]) and val[0, 6] == -np.inf


def test_hubness_requires_matching_arrays():
    with pytest.raises(ValueError):
        hub_of([1, 2], [1], k=1, n_queries=2)


def test_topk_entry_points_refuse_bad_arguments_before_any_launch():
    lib = hip.lib()                                            # host-side checks: no device needed
    EINVAL = hip.NR_EINVAL
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    for k in (0, 129, -1):
        assert lib.nr_slab_topk_rows(p, 4, 8, k, p, p, None) == EINVAL
        assert lib.nr_slab_topk_cols(p, 4, 8, 0, k, p, p, None) == EINVAL
        assert lib.nr_topk_merge(2, p, p, 8, k, p, p, None) == EINVAL
        assert lib.nr_topk_occurrences(p, 4, k, 8, p, p, p, p, None) == EINVAL
    # null pointers
    assert lib.nr_slab_topk_rows(None, 4, 8, 5, p, p, None) == EINVAL
    assert lib.nr_slab_topk_rows(p, 4, 8, 5, None, p, None) == EINVAL
    assert lib.nr_slab_topk_rows(p, 4, 8, 5, p, None, None) == EINVAL
    assert lib.nr_slab_topk_cols(None, 4, 8, 0, 5, p, p, None) == EINVAL
    assert lib.nr_slab_topk_cols(p, 4, 8, 0, 5, None, p, None) == EINVAL
    assert lib.nr_slab_topk_cols(p, 4, 8, 0, 5, p, None, None) == EINVAL
    assert lib.nr_topk_merge(2, None, p, 8, 5, p, p, None) == EINVAL
    assert lib.nr_topk_merge(2, p, None, 8, 5, p, p, None) == EINVAL
    assert lib.nr_topk_merge(2, p, p, 8, 5, None, p, None) == EINVAL
    assert lib.nr_topk_merge(2, p, p, 8, 5, p, None, None) == EINVAL
    assert lib.nr_topk_occurrences(None, 4, 5, 8, p, p, p, p, None) == EINVAL
    assert lib.nr_topk_occurrences(p, 4, 5, 8, None, p, p, p, None) == EINVAL
    assert lib.nr_topk_occurrences(p, 4, 5, 8, p, None, p, p, None) == EINVAL
    assert lib.nr_topk_occurrences(p, 4, 5, 8, p, p, None, p, None) == EINVAL
    assert lib.nr_topk_occurrences(p, 4, 5, 8, p, p, p, None, None) == EINVAL
    # empty or negative extents
    assert lib.nr_slab_topk_rows(p, 0, 8, 5, p, p, None) == EINVAL
    assert lib.nr_slab_topk_cols(p, 4, 8, -1, 5, p, p, None) == EINVAL
    assert lib.nr_topk_merge(0, p, p, 8, 5, p, p, None) == EINVAL
    assert lib.nr_topk_occurrences(p, -1, 5, 8, p, p, p, p, None) == EINVAL


def test_topk_entry_points_are_declared_and_bound():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nr_hip.h")).read()
    for name in ("nr_slab_topk_rows", "nr_slab_topk_cols", "nr_topk_merge", "nr_topk_occurrences"):
        assert f"int {name}(" in header and name in hip.exported_symbols()
    assert hip.ABI_VERSION == 5 and hip.version() == 5
