"""GPU: the exhaustive test-time correction kernels give the pinned bits (slab_kernels_ref.py, golden/slab_kernels.json): every
entry point of nr_hubnorm.hip, nr_sinknorm.hip, nr_localscale.hip and the two applies of nr_mutualprox.hip, at the shapes, layouts
and betas listed there.  The digests were recorded before the kernels moved onto the shared skeletons of csrc/nr_slab.h."""
import pytest

import slab_kernels_ref as K

pytestmark = pytest.mark.gpu


def test_every_pair_is_pinned_and_nothing_else():
    assert sorted(K.pinned()) == sorted(f"{family}/{case}" for family, case in K.pairs())


@pytest.mark.parametrize("family,case", sorted(K.pairs(), key=lambda fc: (fc[1], fc[0])))     # by case: its inputs are drawn once
def test_outputs_have_the_pinned_bits(family, case):
    want = K.pinned()[f"{family}/{case}"]
    got = K.record(family, case)
    assert got["inputs"] == want["inputs"], "the input generator drifted: the pinned outputs do not apply"
    differ = sorted(name for name in set(got["outputs"]) | set(want["outputs"]) if got["outputs"].get(name) != want["outputs"].get(name))
    print(f"{family} at {case}: {len(got['outputs'])} outputs, {len(differ)} differ from the pinned bits")
    assert not differ, differ
