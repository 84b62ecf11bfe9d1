"""The exemplar wrappers on the MI355X with their real engine binding: what they pickle against the recorded states of
tests/golden/make_exemplar_states.py (tests/test_exemplar_cpu.py checks the same without _bind)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_exemplar_states as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["gem", "rehearsal", "icarl"])
def test_bound_wrapper_pickles_the_recorded_keys(name):
    """Nothing that _bind creates leaks into the pickle, and nothing recorded is missing."""
    from clsurvey_amd.methods.gem import GemNet, extend_head
    from clsurvey_amd.methods.icarl import IcarlNet
    from clsurvey_amd.methods.rehearsal import RehearsalNet, replace_head
    shape = (3, 8, 8)
    if name == "gem":
        w = GemNet(extend_head(G.make_net(), 8), 8, 2, [4, 4], 3, lr=0.01, batch_size=4, in_shape=shape)
    elif name == "rehearsal":
        w = RehearsalNet(replace_head(G.make_net(), 8), 8, 2, [4, 4], 3, 0.01, 0.0, False, 6, shape)
    else:
        w = IcarlNet(G.make_net(), 8, 2, [4, 4], 4, 0.01, 0.0, 1.0, 6, shape)
    recorded = torch.load(os.path.join(HERE, "golden", "exemplar_state_%s.pt" % name), weights_only=False)
    assert set(w.__getstate__()) == set(recorded)
