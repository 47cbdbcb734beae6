"""The comparison of tests/form_ladder.py (e_hip <= max(3 x e_cpu, floor) on relative L2 and on max-abs / the 99.9th percentile) bites
where it has to, on synthetic tensors of the largest rung's shapes -- no GPU involved: `hip` and `cpu` are the fp64 reference plus
fp32-rounding-sized noise, and `hip` carries one planted error at a time."""
import torch

import form_ladder as L

EPS = 2.0 ** -24            # half an ulp of fp32 at 1.0: the relative size of one rounding


def _noisy(ref, seed):
    """ref with an independent relative error of a few fp32 roundings per element, stored as fp32 like a real result"""
    g = torch.Generator().manual_seed(seed)
    return (ref * (1.0 + 4.0 * EPS * torch.randn(ref.shape, generator=g, dtype=torch.float64))).float()


def test_ladder_comparison_bites_where_a_norm_cannot():
    g = torch.Generator().manual_seed(0)
    n, c, h, w = max(L.LADDER["segmentation_decoder"])[0], 4, 256, 256      # the output of the largest rung: 32 x 4 x 256 x 256 logits
    ref = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) * 3.0
    cpu, hip = _noisy(ref, 1), _noisy(ref, 2)
    assert L.judge("output", "logits", hip, cpu, ref) == []                 # rounding-sized noise on both sides passes ...
    assert L.judge("dx", "as a gradient", hip, cpu, ref) == []
    # one 4x16-pixel tile (the smallest conv tile) of one image off by 1e-4 of max|ref|: 256 of 8.4 M elements -- the relative L2 error
    # stays at 3e-6, the max-abs error is 1e-4
    tile = hip.clone()
    tile[17, :, 100:104, 48:64] += 1e-4 * float(ref.abs().max())
    bad = L.judge("output", "tile", tile, cpu, ref)
    assert any("[output, max]" in b for b in bad), bad
    assert L.errors(tile, ref)["l2"] < 1e-5                # (a norm alone ranks it next to rounding noise)
    # two swapped output channels
    swap = hip.clone()
    swap[:, [1, 2]] = swap[:, [2, 1]]
    assert len(L.judge("output", "swapped channels", swap, cpu, ref)) == 2  # both metrics
    # a weight gradient with its 3x3 tap grid transposed (128 -> 128, the deepest layers of the largest encoder rung)
    wref = torch.randn(128, 128, 3, 3, generator=g, dtype=torch.float64) * 0.05
    wcpu, whip = _noisy(wref, 3), _noisy(wref, 4)
    assert L.judge("conv_weight", "dW", whip, wcpu, wref) == []
    assert len(L.judge("conv_weight", "dW with kh and kw swapped", whip.transpose(2, 3), wcpu, wref)) == 2
    # a gradient perturbed at a handful of elements (a LeakyReLU slope tie downstream of one pixel) passes the percentile metric that
    # gradients get, and would not pass the max-abs metric of the outputs
    tie = hip.clone()
    tie[3, 2, 40:43, 40:43] += 1e-3 * float(ref.abs().max())
    assert L.errors(tie, ref)["q999"] < 3.0 * L.errors(cpu, ref)["q999"] and L.errors(tie, ref)["max"] > 100.0 * L.errors(cpu, ref)["max"]


def test_ladder_tables_are_consistent():
    """every rung has its id record, ladders are sorted by pixel count, a floor per class and metric, mode-B rungs are on the ladder"""
    for name in L.NETS:
        rungs = L.LADDER[name]
        assert rungs == sorted(rungs, key=lambda r: r[0] * r[1] * r[2]) and len(set(rungs)) == len(rungs), name
        assert L.MODE_B_RUNG[name] in rungs
        assert set(L.RUNG_NEW[name]["train"]) == {L.rung_id(r) for r in rungs}, name
        assert set(L.RUNG_NEW[name].get("eval", {})) == {L.rung_id(r) for r in L.EVAL_LADDER.get(name, [])}, name
        ids = [i for kind in L.RUNG_NEW[name].values() for new in kind.values() for i in new]
        assert len(ids) == len(set(ids)) and all(i.startswith("conv_") for i in ids), name      # first reached at ONE rung
    for cls in L.CLASSES:
        assert set(L.FLOORS[cls]) == {"l2", L.SECOND[cls]} and all(0.0 < v < 1e-1 for v in L.FLOORS[cls].values()), cls
