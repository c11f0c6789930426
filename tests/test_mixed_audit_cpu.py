"""What the bars of tests/mixed_audit.py mean, shown on the CPU with the float64 reference and its fp32 stand-in alone: the stand-in's own
rounding stays 10x below the fp32-valued bar and within the 16-bit condition at every case, and a stand-in with one modelled defect breaks
the audit by 5x the bar or more -- while the whole-step bars against the fp32 step (printed beside it: the same defect in a plain
two-block float64 step) let three of the four through in bf16 and two in fp16."""
import pytest
import torch

import mixed_audit as A

PRECS = ["fp16", "bf16"]
OLD_BARS = {"fp16": 1e-2, "bf16": 1.3e-1}       # per parameter, rel-L2, against the fp32 step (tests/test_train_gpu.py and its kin)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case,storage,attn", A.RUNS, ids=["-".join(r) for r in A.RUNS])
def test_standin_noise_is_ten_times_below_the_bar(case, storage, attn, prec):
    res = A.audit(A.standin_step(case, prec, storage, attn), case, prec, storage, attn)
    print(f"{case} {prec} {storage} {attn}: {A.worst(res)}")
    assert max(res["f32"].values()) <= A.NOISE and A.BAR >= 10 * A.NOISE, max(res["f32"], key=res["f32"].get)
    assert not A.failures(res, prec, storage, A.BAR)
    for k, (ulp, share, off) in res["t16"].items():             # the 16-bit condition, spelt out: the inputs keep the stand-in inside it
        assert off == 0 and share <= A.SHARE, (k, ulp, share, off)
    saved16 = {k.split(".", 1)[1] for k in res["t16"]}                 # which saved tensors the mode keeps in T (`a` goes by the attention bars)
    ffn = {"x12", "h"} if case == "swiglu" else {"hpre", "hact"}
    assert saved16 == (set() if attn == "stored" else {"qkv16"} if storage == "fp32" else {"xn1", "qkv16", "br1", "xn2", "br2"} | ffn)


def _plain_displacement(mutant, T):
    """Worst per-parameter rel-L2 displacement of the defect in a plain two-block float64 step (no rounding but the defect's own): what
    the whole-step comparisons with the fp32 step would have seen of it."""
    make, (case, _, _) = A.MUTANTS[mutant]
    clean = A.standin_step(case, None, "fp32", "stored", dt=torch.float64)["grads"]
    with make(T):
        mut = A.standin_step(case, None, "fp32", "stored", dt=torch.float64)["grads"]
    errs = {k: float((mut[k] - clean[k]).norm() / clean[k].norm()) for k in clean}
    worst = max(errs, key=errs.get)
    return errs[worst], worst


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mutant", list(A.MUTANTS))
def test_mutant_breaks_the_audit_by_five_bars(mutant, prec):
    from test_attn_train_gpu import BWD_BARS
    make, (case, storage, attn) = A.MUTANTS[mutant]
    T = A.DT[prec]
    with make(T):
        rec = A.standin_step(case, prec, storage, attn)
    res = A.audit(rec, case, prec, storage, attn)
    f = max(res["f32"], key=res["f32"].get)
    line = f"{mutant} {prec}: f32 worst {res['f32'][f]:.2e} ({f}) = {res['f32'][f] / A.BAR:.0f} bars, {len(A.failures(res, prec, storage, A.BAR))} entries fail"
    if mutant == "dq_scale_dropped":
        dq = max(e for k, e in res["attn"].items() if k.endswith(".dQ"))
        print(f"{line}; dQ rel-L2 {dq:.2f} against BWD_BARS {BWD_BARS[prec]:g}")
        assert dq >= 5 * BWD_BARS[prec]
        return
    moved, where = _plain_displacement(mutant, T)
    print(f"{line}; in a plain 2-block float64 step it moves {where} by {moved:.2e}: the old bar {OLD_BARS[prec]:g} "
          f"{'passes' if moved < OLD_BARS[prec] else 'fails'} it")
    assert res["f32"][f] >= 5 * A.BAR


def test_audit_guards():
    """A clean record passes; one element of one saved 16-bit tensor moved by 2 ulp, or one gradient entry by 2 bars, does not."""
    case, storage, attn, prec = "ls_reg", "16bit", "flash", "fp16"
    rec = A.standin_step(case, prec, storage, attn)
    assert not A.failures(A.audit(rec, case, prec, storage, attn), prec, storage, A.BAR)
    br1 = rec["blocks"][0]["br1"]
    i = int(br1.float().abs().argmax())
    bits = br1.view(torch.int16).view(-1)
    bits[i] += 2
    bad = A.failures(A.audit(rec, case, prec, storage, attn), prec, storage, A.BAR)
    assert any(b.startswith("b0.br1 1 elements off") for b in bad), bad
    bits[i] -= 2
    g = rec["grads"]["encoder.blocks.0.ls1.gamma"]
    g[3] += 2 * A.BAR * float(g.abs().max())
    bad = A.failures(A.audit(rec, case, prec, storage, attn), prec, storage, A.BAR)
    assert len(bad) == 1 and bad[0].startswith("encoder.blocks.0.ls1.gamma"), bad
