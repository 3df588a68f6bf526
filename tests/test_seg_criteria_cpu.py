"""CPU: the surface of the segmentation criteria (paif_amd/core/loss.py: OhemCELoss, SoftmaxFocalLoss, NormalLoss), their refusals,
the fixtures of tools/make_golden_seg_criteria.py, the restatement tests/seg_criteria_eager.py that the GPU tests lean on, and the
dispatch of `_CompositeBase._seg_term`."""
import inspect
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from paif_amd import ops
from paif_amd.core import loss as L
from paif_amd.core import model_fusion_auto as M
from tests import seg_criteria_eager as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ("1x9x1x1_1x1", "1x9x3x5_12x20", "2x9x6x8_24x32", "1x19x5x7_13x29", "2x3x8x8_8x8", "1x32x4x4_16x16", "2x9x17x33_68x132",
        "2x9x6x8_24x32_ign7")
FAMILY_KIND = {"ohem": "ohem", "focal": "focal", "normal": "normal"}
# constructor signatures of the reference (core/loss.py:343, 362, 376)
INIT = {"OhemCELoss": ["self", "thresh", "n_min", "ignore_lb", "args", "kwargs"],
        "SoftmaxFocalLoss": ["self", "gamma", "ignore_lb", "args", "kwargs"],
        "NormalLoss": ["self", "ignore_lb", "args", "kwargs"]}


def case_kwargs(fx, family, case):
    if family == "ohem":
        return dict(T=float(fx[case + "/T"]), n_min=int(fx[case + "/n_min"]))
    if family == "focal":
        return dict(gamma=float(fx[case + "/gamma"]))
    return {}


def test_signatures_state_dict_and_T():
    for name, params in INIT.items():
        cls = getattr(L, name)
        sig = inspect.signature(cls.__init__)
        assert list(sig.parameters) == params, name
        assert sig.parameters["ignore_lb"].default == 255, name
        assert list(inspect.signature(cls.forward).parameters) == ["self", "logits", "labels"], name
        assert cls.takes_seg_map is True and callable(cls.from_seg_map), name
    mods = [L.OhemCELoss(0.7, 100), L.OhemCELoss(thresh=0.7, n_min=5, ignore_lb=7, extra=1), L.SoftmaxFocalLoss(2.0, 255, "x"), L.NormalLoss()]
    for m in mods:
        assert isinstance(m, torch.nn.Module) and len(m.state_dict()) == 0 and not list(m.parameters()) and not list(m.buffers())
    assert mods[1].ignore_lb == 7 and mods[1].n_min == 5 and mods[2].gamma == 2.0


@pytest.mark.parametrize("case,thresh", [("A", 0.7), ("Bpos", 0.02), ("thresh1", 1.0)])
def test_T_is_the_reference_float32_value(golden, case, thresh):
    fx = golden("gc_seg_ohem_1x9x3x5_12x20")
    assert float(fx[case + "/thresh"]) == thresh
    m = L.OhemCELoss(thresh, 3)
    assert type(m.thresh) is float and m.T == m.thresh
    assert np.float32(m.thresh) == fx[case + "/T"] and m.thresh == float(fx[case + "/T"])
    assert m.thresh == E.ohem_T(thresh)


def test_exports_of_both_core_packages():
    import paif_amd.core as C

    names = sorted(INIT)
    assert all(getattr(C, n) is getattr(L, n) for n in names)
    code = ("import core, paif_amd.core.loss as N; from core import %s;"
            "assert all(getattr(core, n) is getattr(N, n) for n in %r); print('ok')" % (", ".join(names), names))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "paif_amd", "dropin"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0 and b"ok" in r.stdout, r.stdout.decode(errors="replace")


def test_refusals():
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            L.OhemCELoss(bad, 4)
    for bad in (-1.0, -1e-3, float("nan")):
        with pytest.raises(ValueError):
            L.SoftmaxFocalLoss(bad)
    L.OhemCELoss(1.0, 4), L.SoftmaxFocalLoss(0.0)
    logits, labels = torch.zeros(1, 3, 4, 5), torch.zeros(1, 4, 5, dtype=torch.long)
    for n_min in (0, -1, 21):                                       # n = 20 pixels: refused at the call, before the device is asked for
        with pytest.raises(ValueError):
            L.OhemCELoss(0.7, n_min)(logits, labels)
        with pytest.raises(ValueError):
            L.OhemCELoss(0.7, n_min).from_seg_map(torch.zeros(1, 3, 2, 2), labels)
    with pytest.raises(ValueError):
        ops.seg_criterion(logits, labels, "focal", gamma=-0.5)
    with pytest.raises(ValueError):
        ops.seg_criterion(logits, labels, "dice")
    # CPU tensors: there is no CPU path
    for m in (L.OhemCELoss(0.7, 20), L.SoftmaxFocalLoss(2.0), L.NormalLoss()):
        with pytest.raises(RuntimeError, match="no CPU path"):
            m(logits, labels)
    with pytest.raises(ValueError):
        L.NormalLoss()(torch.zeros(1, 3, 2, 2), labels)             # forward is the full-resolution call
    with pytest.raises(TypeError):
        ops.seg_criterion(logits, labels.int(), "normal")
    # C = 33: a direct call raises, whatever the device
    with pytest.raises(NotImplementedError):
        ops.seg_criterion(torch.zeros(1, 33, 4, 5), labels, "normal")
    with pytest.raises(NotImplementedError):
        L.NormalLoss().from_seg_map(torch.zeros(1, 33, 2, 2), labels)


def test_more_than_32_classes_take_the_torch_route():
    """C = 33: `forward` is plain torch (any device) and states what the restatement states."""
    g = torch.Generator().manual_seed(5)
    logits = 2.0 * torch.randn(2, 33, 6, 7, generator=g, dtype=torch.float64)
    labels = torch.randint(0, 33, (2, 6, 7), generator=g)
    labels[0, 2] = 255
    l = E.per_pixel(logits, labels).flatten()
    cnt = int((l > E.ohem_T(0.7)).sum())
    for m, kind, kw in ((L.NormalLoss(), "normal", {}), (L.SoftmaxFocalLoss(2.0), "focal", dict(gamma=2.0)),
                        (L.OhemCELoss(0.7, cnt // 2), "ohem", dict(T=E.ohem_T(0.7), n_min=cnt // 2)),
                        (L.OhemCELoss(0.7, cnt + 3), "ohem", dict(T=E.ohem_T(0.7), n_min=cnt + 3))):
        want = E.criterion(logits, labels, kind, **kw)
        got = m(logits, labels)
        assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want)), (kind, kw, float(got), float(want))
    with pytest.raises(ValueError):
        L.OhemCELoss(0.7, 2 * 6 * 7 + 1)(logits, labels)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_equals_the_committed_float64_results(golden, tag):
    for family, kind in FAMILY_KIND.items():
        fx = golden("gc_seg_%s_%s" % (family, tag))
        seg, lab, ign = torch.from_numpy(fx["seg_map"]), torch.from_numpy(fx["labels"]), int(fx["ignore_lb"])
        assert lab.dtype == torch.int64 and seg.dtype == torch.float32
        assert tag.startswith("%dx%dx%dx%d_%dx%d" % (tuple(seg.shape) + tuple(lab.shape[1:])))
        l64 = E.per_pixel(E.upsample(seg.double(), lab.shape[1:]), lab, ign).numpy()
        assert np.array_equal(l64, fx["l64"])
        for case in fx["cases"]:
            kw = case_kwargs(fx, family, case)
            v, g = E.value_and_grad(seg, lab, kind, ignore_lb=ign, **kw)
            ref_v, ref_g = float(fx[case + "/value64"]), fx[case + "/dseg64"]
            assert abs(float(v) - ref_v) <= 1e-12 * max(1.0, abs(ref_v)), (family, case)
            assert np.abs(g.numpy() - ref_g).max() <= 1e-12 * np.abs(ref_g).max(), (family, case)
            if family == "ohem":
                # the stored regime and margins are those of the stored l
                T, n_min, valid = float(fx[case + "/T"]), int(fx[case + "/n_min"]), fx["labels"] != ign
                mode = E.ohem_mode(torch.from_numpy(l64).flatten(), T, n_min)
                assert {"A": 1, "B": 2}[mode[0]] == int(fx[case + "/mode"]), case
                m = float(fx["margin"])
                assert m >= 1e-4 and m >= 6.0 * float(fx["floor_l"])
                assert float(np.abs(l64[valid] - T).min()) == float(fx[case + "/margin_T"]) >= m, case
                if mode[0] == "B" and float(mode[1]) > 0:
                    assert float(fx[case + "/margin_v"]) >= m, case


def test_the_regimes_the_shapes_are_there_for(golden):
    """Every multi-pixel shape holds mode A, mode B with v > 0 and mode B with v = 0."""
    for tag in TAGS[1:]:
        fx = golden("gc_seg_ohem_" + tag)
        assert int(fx["A/mode"]) == 1 and int(fx["thresh1/mode"]) == 1 and int(fx["nmin1/mode"]) == 1, tag
        assert int(fx["Bpos/mode"]) == 2 and float(fx["Bpos/v"]) > 0, tag
        assert int(fx["Bzero/mode"]) == 2 and float(fx["Bzero/v"]) == 0, tag
        assert int(fx["nminN/mode"]) == 2 and float(fx["nminN/v"]) == 0 and int(fx["nminN/n_min"]) == fx["labels"].size, tag
        ign = fx["labels"] == int(fx["ignore_lb"])
        assert 0.1 < ign.mean() < 0.3 and ign[0, fx["labels"].shape[1] // 2].all(), tag


def test_seg_term_dispatch(monkeypatch):
    """A plain CrossEntropyLoss keeps ops.upsample_ce, the three criteria go to from_seg_map (C <= 32), anything else -- and the three
    criteria above 32 classes -- keeps the torch route."""
    calls = []
    monkeypatch.setattr(ops, "upsample_ce", lambda seg, lab, ignore_index=255: calls.append(("upsample_ce", ignore_index)) or torch.tensor(1.0))
    monkeypatch.setattr(ops, "seg_criterion", lambda seg, lab, kind, **kw: calls.append(("seg_criterion", kind, kw)) or torch.tensor(2.0))
    seg_map, labels = torch.zeros(1, 9, 2, 3), torch.zeros(1, 8, 12, dtype=torch.int32)

    def term(crit, sm=seg_map):
        return M._CompositeBase._seg_term(types.SimpleNamespace(seg_loss=crit), sm, labels)

    assert float(term(torch.nn.CrossEntropyLoss(ignore_index=255))) == 1.0 and calls.pop() == ("upsample_ce", 255)
    assert float(term(L.OhemCELoss(0.7, 10, ignore_lb=7))) == 2.0
    assert calls.pop() == ("seg_criterion", "ohem", dict(ignore_index=7, T=E.ohem_T(0.7), n_min=10))
    assert float(term(L.SoftmaxFocalLoss(0.5))) == 2.0 and calls.pop() == ("seg_criterion", "focal", dict(ignore_index=255, gamma=0.5))
    assert float(term(L.NormalLoss())) == 2.0 and calls.pop() == ("seg_criterion", "normal", dict(ignore_index=255))

    class Foreign(torch.nn.Module):
        def forward(self, up, lab):
            calls.append(("foreign", tuple(up.shape), lab.dtype))
            return up.sum()

    term(Foreign())
    assert calls.pop() == ("foreign", (1, 9, 8, 12), torch.int64)
    term(torch.nn.CrossEntropyLoss(label_smoothing=0.1))          # not the plain criterion: torch route, no fused call
    assert not calls
    v = term(L.NormalLoss(), torch.zeros(1, 33, 2, 3))            # 33 classes: torch route, log(33) per pixel
    assert not calls and abs(float(v) - float(np.log(33.0))) < 1e-6
