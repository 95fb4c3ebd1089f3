"""Register / scratch budgets of the FlowCalc glue kernels (csrc/flowcalc.hip), read from the hipcc listing with the
flags fresco_amd/csrc/Makefile builds them with (no GPU needed): nothing spills, nothing touches scratch memory."""
import shutil

import pytest

from test_kernel_resources_guides import HIPCC, _listing

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


def test_flowcalc_kernels_do_not_spill(tmp_path, monkeypatch):
    import test_kernel_resources_guides as G
    monkeypatch.setitem(G.EXTRA, "flowcalc.hip", ["-ffp-contract=off"])
    k = _listing("flowcalc.hip", tmp_path)
    for pat in ("fc_input", "fc_output"):
        hits = [n for n in k if pat in n]
        assert hits, (pat, sorted(k))
        for n in hits:
            assert k[n]["spill"] == 0 and k[n]["scratch"] == 0, (n, k[n])
            assert k[n]["vgpr"] + k[n]["agpr"] <= 64, (n, k[n])
