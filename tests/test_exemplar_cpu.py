"""The exemplar wrappers (GemNet, RehearsalNet, IcarlNet over methods/exemplar.py) without a GPU: their pickles against
the states recorded from the commit before the shared base (tests/golden/make_exemplar_states.py), and the slab compaction."""
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _cls(name):
    from clsurvey_amd.methods import gem, icarl, rehearsal
    return {"gem": gem.GemNet, "rehearsal": rehearsal.RehearsalNet, "icarl": icarl.IcarlNet}[name]


@pytest.mark.parametrize("name", ["gem", "rehearsal", "icarl"])
def test_pickles_cross_load_with_the_recorded_states(name, monkeypatch):
    """A state recorded from the earlier classes (2 tasks, 3x8x8 store; make_exemplar_states.py --cpu) loads through __setstate__ (the engine part, _bind,
    needs a device and is left out), and __getstate__ of the loaded wrapper yields the same keys and the same stored rows:
    either version reads the other's pickles."""
    cls = _cls(name)
    recorded = torch.load(os.path.join(HERE, "golden", "exemplar_state_%s.pt" % name), weights_only=False)
    assert recorded["observed_tasks"] == [0, 1] and tuple(recorded["in_shape"]) == (3, 8, 8)
    monkeypatch.setattr(cls, "_bind", lambda self: None)
    w = cls.__new__(cls)
    w.__setstate__(dict(recorded, device="cpu"))
    assert w.opt is None
    state = w.__getstate__()
    assert set(state) == set(recorded)
    rows = [k for k in recorded if k.startswith("_rows_")]
    assert sorted(rows) == {"gem": [], "rehearsal": ["_rows_x", "_rows_y"], "icarl": ["_rows_t", "_rows_x"]}[name]
    for k in rows:
        assert recorded[k].shape[0] > 0 and torch.equal(state[k], recorded[k]), k
    for k in set(recorded) - set(rows) - {"net", "device"}:
        v = recorded[k]
        assert torch.equal(state[k], v) if torch.is_tensor(v) else state[k] == v, k


def test_compact_blocks_matches_a_copy():
    """Blocks of 7 rows to blocks of 3, 5 and 6 rows (gaps shorter and longer than the pieces kept), two tensors at once."""
    from clsurvey_amd.methods.exemplar import compact_blocks
    for new, keeps in ((3, [3, 2, 0, 3]), (5, [5, 5, 1, 4]), (6, [6, 6, 6, 6]), (7, [7, 1, 7, 0])):
        a = torch.arange(28 * 2, dtype=torch.float32).view(28, 2)
        b = torch.arange(28)
        a0, b0 = a.clone(), b.clone()
        compact_blocks((a, b), 7, new, keeps)
        for k, keep in enumerate(keeps):
            assert torch.equal(a[k * new:k * new + keep], a0[k * 7:k * 7 + keep]), (new, k)
            assert torch.equal(b[k * new:k * new + keep], b0[k * 7:k * 7 + keep]), (new, k)
