"""The ExpQ acting policy without a GPU: the three native exports and the argument checks of
agents.actors.ExpQWeightedPolicy, which come before anything touches a learner."""

import ctypes

import pytest

from acme_amd import _lib
from acme_amd.agents.actors import ExpQWeightedPolicy


@pytest.mark.parametrize("kind", ["mpo", "dmpo", "crr"])
def test_exports(kind):
    name = f"acme_{kind}_act"
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    # A null handle is refused before any launch, and the message says what was wrong.
    args = _lib.ExpqActArgs()
    assert getattr(_lib.lib(), name)(None, ctypes.byref(args), None) == _lib.ACME_ERR_INVALID
    assert b"null" in _lib.lib().acme_last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(beta=0.0), "beta must be positive"),
    (dict(beta=-1.0), "beta must be positive"),
    (dict(num_action_samples=0), r"num_action_samples must be in \[1, 64\]"),
    (dict(num_action_samples=65), r"num_action_samples must be in \[1, 64\]"),
    (dict(), "takes a CRRLearner, MPOLearner or DistributionalMPOLearner, not a object"),
])
def test_policy_argument_checks(kw, msg):
    with pytest.raises(ValueError, match=msg):
        ExpQWeightedPolicy(object(), **kw)


def test_package_export():
    import acme_amd.agents.crr as crr
    assert crr.ExpQWeightedPolicy is ExpQWeightedPolicy
