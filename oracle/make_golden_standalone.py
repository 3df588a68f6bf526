"""TEST INFRASTRUCTURE -- the fixtures that let the reference-comparison tests run without the reference tree.  Run ONLY where
the reference tree is available (oracle/ref_import.py):   python oracle/make_golden_standalone.py

Same rules as oracle/make_golden.py: imports the real reference (oracle/ref_import.py + oracle/shims), formula weights and inputs
(paif_amd/synthetic.py), stores the REFERENCE's outputs as data.

gs_dataset_items: the reference's `TaskFusion_dataset2.Fusion_dataset('val', ...)` items (vis, ir, label, name) on the synthetic PNG set
    tests/test_dataset.py writes (grey and colour IR files) -- pins paif_amd.TaskFusion_dataset2 (tests/test_dataset.py).
gs_entry_script_imports.json: the (module, name) pairs of the module-level imports of test_original.py / robust_test.py that fall in the
    ported scope -- pins the drop-in import surface (tests/test_dropin_imports.py).
gs_model_forward_ragged: the reference's `Network_MM_Searched` (mit_b0, formula weights and head) on two ragged batches that are not in
    the other goldens -- pins the oracle's whole-model restatement (tests/test_oracle_vs_reference.py).
"""
import ast
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from oracle.make_golden import OUT, npy, save, t  # noqa: E402
from oracle import paif_oracle as O  # noqa: E402
from paif_amd import synthetic as S  # noqa: E402
from tests.helpers import model_sd  # noqa: E402
from tests.test_dataset import _write_set  # noqa: E402
from tests.test_dropin_imports import IN_SCOPE_ROOTS  # noqa: E402

RAGGED = [(1, 40, 56), (3, 32, 72)]


def dataset_items():
    out = {}
    for colour_ir in (False, True):
        with tempfile.TemporaryDirectory() as d:
            irp, vip, lbp = _write_set(d, colour_ir=colour_ir)
            sys.path[:0] = [ref_import._SHIMS, ref_import.REF_ROOT]
            try:
                sys.modules.pop("TaskFusion_dataset2", None)
                import TaskFusion_dataset2 as R
                ref = R.Fusion_dataset('val', ir_path=irp, vi_path=vip, label_path=lbp)
                items = [ref[i] for i in range(len(ref))]
            finally:
                sys.path.remove(ref_import._SHIMS)
                sys.path.remove(ref_import.REF_ROOT)
                sys.modules.pop("TaskFusion_dataset2", None)
                sys.modules.pop("cv2", None)
        tag = "colour" if colour_ir else "grey"
        for j, name in enumerate(("vis", "ir", "label")):
            out["%s_%s" % (tag, name)] = np.stack([npy(it[j]) for it in items])
        out["%s_name" % tag] = np.array([it[3] for it in items])
    save("gs_dataset_items", **out)


def entry_script_imports():
    pairs = []
    for script in ("test_original.py", "robust_test.py"):
        tree = ast.parse(open(os.path.join(ref_import.REF_ROOT, script), encoding="utf-8").read())
        for node in tree.body:                      # module-level imports only: what runs before main
            if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] in IN_SCOPE_ROOTS:
                pairs += [(node.module, a.name) for a in node.names]
            elif isinstance(node, ast.Import):
                pairs += [(a.name, None) for a in node.names if a.name.split(".")[0] in IN_SCOPE_ROOTS]
    path = os.path.join(OUT, "gs_entry_script_imports.json")
    with open(path, "w") as f:
        json.dump(sorted(set(pairs), key=lambda p: (p[0], p[1] or "")), f, indent=1)
    print("wrote gs_entry_script_imports.json")


def model_forward_ragged():
    R = ref_import.load()
    with ref_import.quiet():
        m = R["mfa"].Network_MM_Searched(32, O.FUSION_AT, None, None, "mit_b0", num_classes=9)
    m.eval()
    S.load_formula_weights(m)
    # the test rebuilds the state_dict from the committed layout (tests/helpers.py model_sd): it must be the reference's own
    sd, mine = m.state_dict(), model_sd("mit_b0")
    assert set(sd) == set(mine)
    assert all(torch.equal(sd[k].to(mine[k].dtype), mine[k]) for k in sd)
    out = {}
    for B, H, W in RAGGED:
        ir, vis, _ = S.make_batch(B, H, W, start=5)
        with torch.no_grad():
            f, s = m(t(ir), t(vis))
        out["fused_%dx%dx%d" % (B, H, W)] = npy(f)
        out["seg_%dx%dx%d" % (B, H, W)] = npy(s)
    save("gs_model_forward_ragged", **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    dataset_items()
    entry_script_imports()
    model_forward_ragged()
