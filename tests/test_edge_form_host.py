"""CPU-only: the edge-form identity of ppbo_posterior (PPBO_FORM_EDGE) in NumPy (tests/probes/edge_form_identity.py)."""
import importlib.util
import os

import pytest

_PROBE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "probes", "edge_form_identity.py")
_spec = importlib.util.spec_from_file_location("edge_form_identity", _PROBE)
probe = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(probe)


@pytest.mark.parametrize("n_q,m,D", [(5, 7, 3), (4, 31, 6), (3, 25, 2)])
def test_edge_form_matches_node_form_and_dense_congruence(n_q, m, D):
    assert probe.check(n_q, m, D) <= 1e-12
