"""CPU model of the large-cloud FPS tier on the short slices of a ragged batch (pn2_farthest_point_sample_large_ragged, DESIGN.md
4.1e "with lengths"). The dense tier never sees fewer than 16385 points; a cloud of a ragged batch may be one point. The numpy
restatement of the tier's rule (_large_fps, tests/test_fps_large_model.py: cell order, groups of L records with tight boxes,
cached group keys, the skip rule asserted in every round) is run on slices of 1 .. 3000 points -- one record, one group, one
record either side of one and of four groups, fewer groups than the kernel has waves -- against the oracle at every group length,
with more samples than points included. The slices are cut from the clouds of the device cases
(tests/fps_large_ragged_cases.py). No GPU."""
import numpy as np
import pytest

from fps_large_ragged_cases import MODEL_KINDS, MODEL_M, MODEL_SIZES, model_slices
from test_fps_large_model import _large_fps


@pytest.mark.parametrize("L", [64, 128, 256])
@pytest.mark.parametrize("kind", sorted(MODEL_KINDS))
def test_the_grouping_rule_on_short_slices(oracle, kind, L):
    slices = model_slices(kind)
    assert [nc for nc, _ in slices] == MODEL_SIZES
    for nc, x in slices:
        assert x.shape == (nc, 3)
        want = oracle.farthest_point_sample(MODEL_M, np.ascontiguousarray(x[None]))[0]
        got, share = _large_fps(x, MODEL_M, L)
        assert np.array_equal(got, want), "%s n_c=%d L=%d: first difference at %s" % (kind, nc, L, np.argwhere(got != want)[:3].ravel())
        assert (got < nc).all()
        if nc < MODEL_M:                                   # an exhausted cloud runs on at value 0: point 0 wins every further round
            assert (got[nc:] == 0).all()
        if kind == "identical" and nc > 1:
            assert share == 1.0                            # every box holds every sample: nothing can be pruned
