"""-m gpu: the d = 128 encoder kernels held to fp64 STAGE BY STAGE in bf16 (tests/bf16_stage_ref.py has the rounding map, the metric and the
bars). Every case runs once, forward and backward; every intermediate the call keeps is read back through the ABI v26 stage hooks
(egot2_amd.functional.EncoderStages) and every stage is recomputed in fp64 from the items the device itself held going into it. Each case
also runs in f32s against the unrounded reference at its own fp32 yardstick: that validates the hooks, the unpacking and the stage
definitions independently of the rounding map. Two negative controls run on the device: the bf16 run against the unrounded reference and
the f32s run against the rounding reference must both miss the QKV and weight-gradient bars by 100x."""
from dataclasses import replace

import pytest
import torch

from tests import bf16_stage_ref as R
from tests import fp32_grade as G

pytestmark = pytest.mark.gpu
CONTROL_MIN = 100.0
FWD_ITEMS = ("XIN", "QKV", "RES1", "X1", "HID", "ALIVE", "RES2", "ATTN_O", "LSE")
BWD_ITEMS = ("G2", "DHID", "G1", "ATTN_O", "DQKV")


def run_device(case, mode, st, sd, data, cuda):
    """Forward and backward of the case in compute `mode` -> ({item name: tensor}, {item: why it is absent}): the items of the stage hooks
    ("XIN0", "DSEG1", ...), "OUT" (logits / rows) and "grad:<parameter>"."""
    from egot2_amd import functional as F_egx
    case = replace(case, compute=mode)
    dev, absent = {}, {}
    with G._env(case.env):
        m = G.new_model(case)
        m.load_state_dict(sd)
        m = m.to(cuda).set_compute(mode, case.impl)
        m.train(True)
        if case.det:
            m.set_deterministic(True)
        if case.wcache:
            m.enable_weight_cache()
        m._egx_seed = lambda: data["seed"]
        cw = torch.tensor(G.CE_W, device=cuda)
        if case.family == "ragged_train":
            feats, lengths = G._pad(data["clips"], cuda, False)
            out, loss = m.forward_features_ragged(*feats, lengths=lengths, target=data["target"].to(cuda), class_weight=cw)
        else:
            feats = [f.to(cuda) for f in data["feats"]]
            if case.loss == "ce_fused":
                out, loss = m.forward_features(*feats, target=data["target"].to(cuda), class_weight=cw)
            else:
                out = m.forward_features(*feats)
                if case.loss == "ce":
                    loss = torch.nn.functional.cross_entropy(out, data["target"].to(cuda), weight=cw)
                else:
                    flat = out.reshape(-1)
                    loss = (flat * (data["w"] if case.loss == "rows" else G.lin_w(flat.numel())).to(cuda).reshape(-1)).sum()
        impl = F_egx.last_encoder_impl()
        assert impl == case.expect, (case.id, impl)
        if case.family in ("perclip", "sliced", "hoi"):
            assert F_egx.last_encoder_slices() == case.slices, (case.id, F_egx.last_encoder_slices())
        hooks = F_egx.EncoderStages(out)

        def read(items, layers):
            for name in items:
                for l in layers:
                    key = f"{name}{l}" if name != "PRE" else "PRE"
                    if key in dev:
                        continue
                    t = hooks.read(name, l)
                    if t is None:
                        absent[key] = "not kept by this implementation (egx_*_stage_info)"
                    else:
                        dev[key] = t.cpu()
        fwd = [i for i in FWD_ITEMS if not (i == "ATTN_O" and st.b.family == "perclip")]
        read(("PRE",), (0,))
        read(fwd, range(case.L))
        loss.backward()
        read(BWD_ITEMS, range(case.L))
        read(("DSEG",), range(len(st.m.proj)))
        torch.cuda.synchronize()
    dev["OUT"] = out.detach().reshape(-1, out.shape[-1]).cpu()
    for k, p in m.named_parameters():
        if p.grad is not None:
            dev["grad:" + k] = p.grad.detach().cpu()
    return dev, absent


_RUNS: dict = {}


def _run(case, mode, cuda):
    """One device run per (case, mode), shared by the tests below; the device items are never written to."""
    key = (case.id, mode)
    if key not in _RUNS:
        st, sd, data = R.setup(case, mode)
        _RUNS[key] = (st,) + run_device(case, mode, st, sd, data, cuda)
    return _RUNS[key]


def _check(case, mode, cuda):
    st, dev, absent = _run(case, mode, cuda)
    worst, detail, notes = R.stage_errors(st, dev)
    # every stage of the plan is checked, or an item it needs is one the hook reports as not kept
    planned = {name for name, _, _ in st.plan()}
    for name in planned - set(worst):
        assert any(n.startswith(name + ":") for n in notes["missing"]), (case.id, mode, name)
    for miss in notes["missing"]:
        assert miss.split(": ")[1] in absent, (case.id, mode, miss)
    # what may be absent is pinned: the log-sum-exp of a per-clip call, nothing of a tiled or ragged one (so that no stage goes unchecked)
    expect = {f"LSE{l}" for l in range(case.L)} if st.b.family == "perclip" else set()
    assert set(absent) == expect and set(worst) == planned, (case.id, mode, sorted(absent), sorted(planned - set(worst)))
    ratio = {k: v / R.bar(k, mode) for k, v in worst.items()}
    print(case.id, mode, {k: f"{v:.2f}" for k, v in ratio.items()}, "alive skipped", f"{notes['alive_skip']:.1e}", "not kept", sorted(absent))
    return ratio, detail, notes


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_bf16_stages_meet_their_bars(egx_lib, cuda, case):
    """compute="bf16": every stage of the case within 8 x the fp32 yardstick of its rounding reference."""
    ratio, detail, notes = _check(case, "bf16", cuda)
    assert notes["alive_bad"] == 0 and notes["alive_skip"] <= R.ALIVE_SKIP_MAX, (case.id, notes)
    bad = {k: round(v, 2) for k, v in ratio.items() if not v <= 1.0}
    assert not bad, (case.id, bad, {k: [(n, f"{e:.2g}") for n, e in detail[k]] for k in bad})


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_f32s_stages_meet_the_unrounded_reference(egx_lib, cuda, case):
    """compute="f32s" against the reference without any rounding: the hooks, the unpacking and the stage definitions on their own."""
    ratio, detail, notes = _check(case, "f32s", cuda)
    assert notes["alive_bad"] == 0 and notes["alive_skip"] <= R.ALIVE_SKIP_MAX, (case.id, notes)
    bad = {k: round(v, 2) for k, v in ratio.items() if not v <= 1.0}
    assert not bad, (case.id, bad, {k: [(n, f"{e:.2g}") for n, e in detail[k]] for k in bad})


CONTROL_IDS = ("pc-t15-l2-p05-one", "pc-s21-l2-cut", "tl-s51", "rt-ttm2-l1")


@pytest.mark.parametrize("cid", CONTROL_IDS)
def test_controls_miss_the_bars(egx_lib, cuda, cid):
    """Negative controls on the device: the bf16 run against the UNROUNDED reference, and the f32s run against the ROUNDING reference, both miss
    the QKV and the weight-gradient bars by 100x: the rounding map is what makes the bf16 comparison pass, and it is not vacuous."""
    case = R.BY_ID[cid]
    for dev_mode, ref_mode in (("bf16", "f32s"), ("f32s", "bf16")):
        _, dev, _ = _run(case, dev_mode, cuda)
        st, _, _ = R.setup(case, ref_mode)
        worst, _, _ = R.stage_errors(st, dev)
        for stage in ("qkv", "wgrad"):
            r = worst[stage] / R.bar(stage, ref_mode)
            print(cid, dev_mode, "against the", ref_mode, "reference:", stage, f"{r:.3g} x bar")
            assert r >= CONTROL_MIN, (cid, dev_mode, ref_mode, stage, r)
