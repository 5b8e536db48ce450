"""-m gpu: decode() over 9 .. 64 target tokens with autograd (DecoderMixin.egx_long_targets: the composed fp32 decoder on
egx_target_attention_fwd / _bwd, csrc/target_attn.hip). Cases, masks, references and bars: tests/long_target_ref.py. Held to:
  1. every LT_ATTN_CASES entry, forward and backward, against the fp64 reference under attn_mask(row_stride=64) at the operator bars, in
     test_gpu_unit_ops.py's buffer layouts: outputs poisoned with NaN first, nothing outside the (row, head column) windows written;
  2. forward and backward repeat bit for bit; with B doubled by repeating the inputs the first half keeps its bits; dq / dk / dv written
     into NaN-filled buffers are finite everywhere (assignment, not accumulation);
  3. every decoder case in train mode under the host seed against g_decode in fp64 under long_decoder_masks: logits, d(memory), every
     decoder / fc / embedding gradient at the composed-f32 bars (logits 1e-3, gradients 1e-2); last_decoder_impl() == "composed_long";
     the step repeats bit for bit under its seed;
  4. the training step as the reference writes it, F.cross_entropy(decode(y, mem).permute(1, 2, 0), target) with -100 padding, at the LTA
     widths: loss within twice the logits bar (a log-probability moves by at most twice the worst logit error), gradients at 1e-2;
  5. eval mode with autograd: logits at the logits bar; rows before a changed token keep their bits;
  6. the pins: switch off -> "outside 1..8" as before; switch on -> 65 tokens refused naming 64, return_attention at 9 tokens refused as
     before, 5 and 8 tokens bit-identical to the switch-off call on the same route, a bf16 model in eval under no_grad still "forced";
  7. an f32 model in eval under no_grad (egx_decoder_forced does not serve it): "composed_long", logits at the logits bar;
  8. memory_lengths= with 12 tokens through _egx_decode_ragged_train: each clip's logits against decode() on its own memory, bound 4 x the
     worst difference measured on the MI355X (RAGGED_VS_OWN_MEASURED), never looser than the logits bar."""
import pytest
import torch
import torch.nn.functional as F

from oracle import translator_ref as tr
from tests import decoder_dropout_gate as ddg
from tests import greedy_ref as gr
from tests import long_target_ref as lt
from tests import unit_ref as ur
from tests.test_gpu_unit_ops import _attn_layout, _check, _nanbuf, _outside_is_nan, _same_bits, _stream, _win

pytestmark = pytest.mark.gpu

RAGGED_VS_OWN_MEASURED = 0.0    # item 8: worst |difference| / max(1, |ref|max) over the three clips, measured on an MI355X


# ---- items 1 and 2: the operator -----------------------------------------------------------------------------------------------------------
def _run_attention(lib, cuda, ci, reps=1):
    """Case ci with its inputs repeated `reps` times along the batch, laid out as the case's layout says -> (got {q, k, v, o: window
    tensors on the CPU: dq, dk, dv, o}, out buffers, windows, layout, input buffers before / after)."""
    B, H, Sq, Sk, dh, causal, p, layout = lt.LT_ATTN_CASES[ci]
    d, seed, site = H * dh, lt.LT_ATTN_SEED, lt.lt_site(ci)
    host = {n: t.repeat(reps, 1, 1) for n, t in zip(("q", "k", "v", "o"), lt.lt_inputs(ci))}       # "o": d_o, which shares o's geometry
    B = B * reps
    lay = _attn_layout(layout, d)
    rows = {"q": B * Sq, "k": B * Sk, "v": B * Sk, "o": B * Sq}
    win = {n: (lay[n][1], rows[n], lay[n][2], d) for n in lay}
    size = {}
    for n, (bname, off, ld) in lay.items():
        size[bname] = max(size.get(bname, 0), rows[n] * ld)
    inp = {b: _nanbuf(s, cuda) for b, s in size.items()}
    out = {b: _nanbuf(s, cuda) for b, s in size.items()}
    for n in lay:
        _win(inp[lay[n][0]], *win[n]).copy_(host[n].reshape(rows[n], d).to(cuda))
    before = {b: t.clone() for b, t in inp.items()}

    def addr(bufs, n):
        return bufs[lay[n][0]].data_ptr() + 4 * lay[n][1]

    ld = {n: lay[n][2] for n in lay}
    _check(lib, lib.egx_target_attention_fwd(addr(inp, "q"), ld["q"], addr(inp, "k"), ld["k"], addr(inp, "v"), ld["v"], addr(out, "o"), ld["o"],
                                             B, Sq, Sk, H, dh, causal, p, seed, site, _stream()))
    _check(lib, lib.egx_target_attention_bwd(addr(inp, "q"), ld["q"], addr(inp, "k"), ld["k"], addr(inp, "v"), ld["v"], addr(inp, "o"), ld["o"],
                                             addr(out, "q"), addr(out, "k"), addr(out, "v"), B, Sq, Sk, H, dh, causal, p, seed, site, _stream()))
    torch.cuda.synchronize()
    got = {n: _win(out[lay[n][0]], *win[n]).cpu() for n in lay}
    return got, out, win, lay, inp, before


_OP_REF = {}


def _op_ref(ci):
    if ci not in _OP_REF:
        o, (dq, dk, dv) = lt.lt_eval(ci, torch.float64)
        _OP_REF[ci] = {"o": o, "q": dq, "k": dk, "v": dv}
    return _OP_REF[ci]


@pytest.mark.parametrize("ci", range(len(lt.LT_ATTN_CASES)), ids=[lt.lt_case_id(c) for c in lt.LT_ATTN_CASES])
def test_target_attention_fwd_bwd(egx_lib, cuda, ci):
    B, H, Sq, Sk, dh, causal, p, layout = lt.LT_ATTN_CASES[ci]
    d, case, ref = H * dh, lt.lt_case_id(lt.LT_ATTN_CASES[ci]), _op_ref(ci)
    got, out, win, lay, inp, before = _run_attention(egx_lib, cuda, ci)
    err = {n: ur.rel_err(got[n], ref[n].reshape(-1, d)) for n in ("o", "q", "k", "v")}
    for n, e in err.items():
        print(f"LONGTARGET target_attention {case} {'o' if n == 'o' else 'd' + n} err {e:.3e} bar {lt.LT_BAR['out' if n == 'o' else 'grad']:.3e}")
    assert err["o"] <= lt.LT_BAR["out"]
    assert max(err[n] for n in "qkv") <= lt.LT_BAR["grad"], err
    # exactly once, and nowhere else: every element outside the addressed (row, head column) windows is still NaN, every one inside finite
    for b in out:
        assert _outside_is_nan(out[b], [win[n] for n in lay if lay[n][0] == b]), f"buffer {b} was written outside its windows"
    for b in inp:
        assert _same_bits(inp[b], before[b]), f"input buffer {b} changed"
    for n in got:
        assert bool(torch.isfinite(got[n]).all()), f"{n}: an element of the NaN-filled output was not assigned"


@pytest.mark.parametrize("ci", range(len(lt.LT_ATTN_CASES)), ids=[lt.lt_case_id(c) for c in lt.LT_ATTN_CASES])
def test_target_attention_bits(egx_lib, cuda, ci):
    B, H, Sq, Sk = lt.LT_ATTN_CASES[ci][:4]
    a = _run_attention(egx_lib, cuda, ci)[0]
    b = _run_attention(egx_lib, cuda, ci)[0]
    two = _run_attention(egx_lib, cuda, ci, reps=2)[0]
    rows = {"q": B * Sq, "k": B * Sk, "v": B * Sk, "o": B * Sq}
    for n in a:
        assert _same_bits(a[n], b[n]), f"{n} does not repeat"
        assert bool(torch.isfinite(two[n]).all())
        assert _same_bits(a[n], two[n][:rows[n]]), f"{n}: the first half's bits depend on B"


# ---- the decoder on the GPU ----------------------------------------------------------------------------------------------------------------
def _model(case, cuda, compute="f32", long_targets=True):
    m = lt.new_model(case)
    m.load_state_dict(lt.case_data(case)["sd"])
    m = m.to(cuda).set_compute(compute)
    m.egx_long_targets = long_targets
    return m


def _step(m, case, data, cuda, seed, y=None, loss=None):
    """One forward and backward of decode() -> the oracle_run layout plus "impl" and "loss"."""
    from egot2_amd import functional as F_egx
    m._egx_seed = lambda: seed
    names = [k for k, _ in m.named_parameters() if ddg.is_decoder_param(k)]
    m.zero_grad(set_to_none=True)
    mem = data["mem"].to(cuda).requires_grad_(True)
    torch.cuda.synchronize()
    ddg._poison(cuda, [mem.numel()] + [p.numel() for k, p in m.named_parameters() if ddg.is_decoder_param(k)])
    logits = m.decode((data["y"] if y is None else y).to(cuda), mem)
    impl = F_egx.last_decoder_impl()
    val = (logits * data["w"].to(cuda)).sum() if loss is None else loss(logits)
    val.backward()
    torch.cuda.synchronize()
    named = dict(m.named_parameters())
    missing = [k for k in names if named[k].grad is None]
    assert not missing, f"no gradient for {missing}"
    return {"logits": logits.detach().clone(), "dmem": mem.grad.detach().clone(), "grads": {k: named[k].grad.detach().clone() for k in names},
            "impl": impl, "loss": val.detach().clone()}


def _same_step(a, b):
    return (torch.equal(a["logits"], b["logits"]) and torch.equal(a["dmem"], b["dmem"])
            and all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"]))


def _say(what, g):
    print(f"LONGTARGET {what}: logits {g['logits']:.3e} dmem {g['dmem']:.3e} grad {g['grad']:.3e} ({g['worst_grad']}) miss {g['miss']:.3g}")


# ---- item 3 ----
@pytest.mark.parametrize("case", lt.LT_DECODER_CASES, ids=[c.id for c in lt.LT_DECODER_CASES])
def test_train_step_matches_the_oracle_under_its_masks(egx_lib, cuda, case):
    data, ref = lt.case_data(case), lt.reference(case)
    m = _model(case, cuda).train()
    a = _step(m, case, data, cuda, case.host_seed)
    b = _step(m, case, data, cuda, case.host_seed)
    g = ddg.gate(a, ref, case.bars)
    _say(f"train {case.id}", g)
    assert a["impl"] == "composed_long"
    assert g["ok"], g["ratio"]
    assert _same_step(a, b), "the step does not repeat bit for bit under its seed"
    if case.p_drop > 0 or case.p_pos > 0:
        assert not torch.equal(a["logits"], _step(m, case, data, cuda, case.host_seed + 1)["logits"])       # another seed: other masks


# ---- item 4 ----
def test_reference_training_step_with_padding(egx_lib, cuda):
    case = lt.LTA_CASE
    data = lt.case_data(case)
    g = torch.Generator().manual_seed(31)
    target = torch.randint(0, case.V, (case.B, case.sy), generator=g)
    target[0, case.sy - 1], target[1, 7] = -100, -100
    ce = lambda logits: F.cross_entropy(logits.permute(1, 2, 0), target.to(logits.device))  # noqa: E731
    # the same expression on the oracle
    sdd = {k: (v.double() if k.endswith(".pe") else v.double().clone().requires_grad_(True)) for k, v in data["dsd"].items()}
    mem = data["mem"].double().clone().requires_grad_(True)
    loss = ce(tr.g_decode(sdd, case.H, data["y"], mem, masks=data["masks"]))
    loss.backward()
    ref = {"logits": loss.detach().reshape(1), "dmem": mem.grad, "grads": {k: v.grad for k, v in sdd.items() if v.requires_grad}}
    res = _step(_model(case, cuda).train(), case, data, cuda, case.host_seed, loss=ce)
    res["logits"] = res["loss"].reshape(1)
    gate = ddg.gate(res, ref, {**case.bars, "logits": 2 * case.bars["logits"]})
    _say("reference training step (loss in the logits column)", gate)
    assert res["impl"] == "composed_long" and gate["ok"], gate["ratio"]


# ---- item 5 ----
def test_eval_mode_with_autograd_and_causality(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    case = lt.LT_BY_ID["d256-sy21"]
    data = lt.case_data(case)
    m = _model(case, cuda).eval()
    mem = data["mem"].to(cuda).requires_grad_(True)
    y = data["y"].to(cuda)
    assert torch.is_grad_enabled()
    logits = m.decode(y, mem)
    assert F_egx.last_decoder_impl() == "composed_long" and logits.requires_grad
    with torch.no_grad():
        ref = tr.g_decode({k: v.double() for k, v in data["dsd"].items()}, case.H, data["y"], data["mem"].double())
    err = (logits.detach().cpu().double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print(f"LONGTARGET eval+autograd {case.id}: logits {err:.3e} bar {case.bars['logits']:.1e}")
    assert err <= case.bars["logits"]
    for t in (9, 20):
        y2 = y.clone()
        y2[:, t] = (y2[:, t] + 1) % case.V
        other = m.decode(y2, mem)
        assert torch.equal(other[:t], logits[:t]), f"rows before token {t} changed"
        assert not torch.equal(other[t], logits[t])


# ---- item 6 ----
def test_pins_hold(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    case = lt.LT_BY_ID["d256-sy9"]
    data = lt.case_data(case)
    mem, y9 = data["mem"].to(cuda), data["y"].to(cuda)
    off = _model(case, cuda, long_targets=False).train()
    off._egx_seed = lambda: case.host_seed
    assert torch.is_grad_enabled()
    with pytest.raises(Exception, match=r"outside 1\.\.8"):
        off.decode(y9, mem)
    on = _model(case, cuda).train()
    y65 = torch.zeros((case.B, 65), dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError, match="64"):
        on.decode(y65, mem)
    on.eval()
    off.eval()
    with torch.no_grad():
        with pytest.raises(Exception) as e_off:
            off.decode(y9, mem, return_attention=True)
        with pytest.raises(Exception) as e_on:
            on.decode(y9, mem, return_attention=True)
    assert type(e_on.value) is type(e_off.value) and str(e_on.value) == str(e_off.value) and "outside 1..8" in str(e_on.value)
    # at most 8 tokens: the switch changes nothing
    on.train()
    off.train()
    for sy in (8, 5):
        y = data["y"][:, :sy]
        d2 = {**data, "w": data["w"][:sy]}
        a, b = _step(off, case, d2, cuda, case.host_seed, y=y), _step(on, case, d2, cuda, case.host_seed, y=y)
        assert a["impl"] == b["impl"] == "composed"
        assert _same_step(a, b), f"sy = {sy}: the switch moved bits"
    # a bf16 model in eval under no_grad: the forced route keeps the call and its bits
    mb, _, _ = gr.hoi_model(256, 8, 2, 40, 95)
    mb = mb.to(cuda).set_compute("bf16").eval()
    memb = torch.randn((16, 3, 256), generator=torch.Generator().manual_seed(5)).to(cuda)
    yb = torch.randint(0, 40, (3, 21), generator=torch.Generator().manual_seed(6)).to(cuda)
    with torch.no_grad():
        want = mb.forced_decode(memb, yb)
        mb.egx_long_targets = True
        got = mb.decode(yb, memb)
        assert F_egx.last_decoder_impl() == "forced" and torch.equal(got, want)


# ---- item 7 ----
def test_f32_model_under_no_grad_takes_the_long_route(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    case = lt.LT_BY_ID["d256-sy21"]
    data = lt.case_data(case)
    m = _model(case, cuda, compute="f32").eval()
    with torch.no_grad():
        logits = m.decode(data["y"].to(cuda), data["mem"].to(cuda))
        assert F_egx.last_decoder_impl() == "composed_long"
        ref = tr.g_decode({k: v.double() for k, v in data["dsd"].items()}, case.H, data["y"], data["mem"].double())
    err = (logits.cpu().double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print(f"LONGTARGET eval no_grad f32 {case.id}: logits {err:.3e} bar {case.bars['logits']:.1e}")
    assert err <= case.bars["logits"]


# ---- item 8 ----
def test_ragged_memory_with_long_targets(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    case = lt.LT_BY_ID["d256-sy21"]
    data = lt.case_data(case)
    lengths, sy = (4, 7, 4), 12
    m = _model(case, cuda).eval()
    g = torch.Generator().manual_seed(41)
    packed = torch.randn((sum(lengths), case.d), generator=g).to(cuda).requires_grad_(True)
    y = torch.randint(0, case.V, (len(lengths), sy), generator=g).to(cuda)
    kw = dict(embedding=m.embedding, pos_embed=m.pos_embed, decoder=m.transformer_decoder, fc=m.fc, n_heads=m.n_heads, p_drop=m.dp_rate)
    out = m._egx_decode_ragged_train(y, packed, torch.tensor(lengths), **kw)
    assert F_egx.last_decoder_impl() == "grouped" and out.shape == (sy, len(lengths), case.V)
    out.sum().backward()
    assert packed.grad is not None and bool(torch.isfinite(packed.grad).all())
    worst, r0 = 0.0, 0
    for b, S_b in enumerate(lengths):
        own = m.decode(y[b:b + 1], packed[r0:r0 + S_b, None, :].detach())
        assert F_egx.last_decoder_impl() == "composed_long"
        worst = max(worst, (out[:, b:b + 1] - own).abs().max().item() / max(1.0, own.abs().max().item()))
        r0 += S_b
    bound = min(4 * RAGGED_VS_OWN_MEASURED, case.bars["logits"])
    print(f"LONGTARGET ragged sy {sy} lengths {lengths}: worst difference {worst:.3e} (recorded {RAGGED_VS_OWN_MEASURED:.3e}, bound {bound:.3e})")
    assert worst <= bound
