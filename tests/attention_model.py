"""A CPU model of the rounding points of ``vface_attention`` (csrc/attention.hip), one (sample, head) at a time, plus seeded
DEFECTS of one line each, and the input families of the attention tests.  It restates the kernel's own comments in torch: it is
not a reference (the reference is the fp64 softmax of ``kernel_bounds.attention_ref_and_bound``) -- it shows that the bound admits
a correct kernel and refuses a subtly wrong one (test_attention_bound_cpu.py), and it is the yardstick of the one aggregate
assertion of test_attention_gpu.py.  Plain module, nothing collected by pytest.

What is modelled: q scaled by fp32(scale * log2 e) and rounded to the 16-bit type once (``form="lazy"`` / ``"spec"``) or the scale
applied to the fp32 scores (``"exact"``); key blocks of 64; the reference set to the first block's maximum, then raised -- with the
rescale of O and of the denominator -- only where a block's maximum exceeds it by more than 8 base-2 units (lazy), never (spec: the
query runs again with the lazy rule when its denominator or an output sum comes out non-finite, as the kernel's second pass does),
or at every new maximum (exact); P rounded to the 16-bit type; O and the denominator in fp32, the denominator from the rounded P
(the instantiations with a spare V column: dh 8, 40) or from the fp32 P (dh 16, 32, 80, 160); one rounding at the end.
Not modelled: the order of the fp32 additions inside an MFMA, v_exp_f32's last bit."""
import torch

KVB = 64
LOG2E = 1.44269504088896340736
DEFECTS = ("tail_unmasked", "no_rescale", "flush_p", "o16", "last_key_dropped")
# test_attention_gpu.py's aggregate assertion at 4096 keys: rel_l2(kernel, fp64) <= AGGREGATE_MARGIN * rel_l2(model, fp64).  Measured
# kernel / model on the MI355X: 1.000 in fp16 and in bf16 (that test's docstring has the figures), + 25 %.  It may never exceed 2: the
# model's 16-bit-O defect sits at 3.2x (fp16) / 3.5x (bf16) of the model, which test_attention_bound_cpu.py asserts against this number.
AGGREGATE_MARGIN = 1.25


def ones_column(dh):
    """True where the instantiation of head dim ``dh`` (value tile width: sets x dh) has a spare V column (DVP > DV): its denominator
    is summed from the ROUNDED P."""
    return (-dh) % 16 != 0


def attention_model(q, k, v, scale, dt, form="lazy", denom_rounded=None, defect=None, sets=1):
    """``q [n, dh]``, ``k, v [nk, dh]`` of type ``dt`` -> ``[n, dh]`` of type ``dt``.  ``sets``: the value sets of the shared-score
    instantiation (2 or 3); one set's output is modelled at a time, so it only selects the denominator form -- the value tile is
    ``sets * dh`` wide and has a spare column where THAT is no multiple of 16 (dh 40 and 8 with 3 sets; not with 2)."""
    assert form in ("lazy", "exact", "spec") and (defect is None or defect in DEFECTS)
    n, dh = q.shape
    nk = k.shape[0]
    if denom_rounded is None:
        denom_rounded = ones_column(sets * dh)
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    qf = q.float() if form == "exact" else (q.float() * c).to(dt).float()
    nb = -(-nk // KVB)
    kp = torch.zeros(nb * KVB, dh)
    vp = torch.zeros(nb * KVB, dh)
    kp[:nk], vp[:nk] = k.float(), v.float()           # rows past nk: the out-of-range loads return zeros
    live = torch.arange(nb * KVB) < (nk - 1 if defect == "last_key_dropped" else nk)
    if defect == "tail_unmasked":
        live[:] = True

    def walk(rows, rule):
        qq = qf[rows]
        m = torch.zeros(len(rows), 1) if rule != "exact" else torch.full((len(rows), 1), -1e30)
        O = torch.zeros(len(rows), dh)
        l = torch.zeros(len(rows), 1)
        for kb in range(nb):
            sl = slice(kb * KVB, (kb + 1) * KVB)
            s = qq @ kp[sl].T
            s = torch.where(live[sl][None, :], s, torch.full_like(s, -1e30))
            if rule == "exact":
                m_new = torch.maximum(m, s.max(dim=1, keepdim=True).values)
                alpha = torch.exp2((m - m_new) * c)
                m = m_new
                p = torch.exp2(s * c - m * c)
            else:
                mx = (s - m).max(dim=1, keepdim=True).values
                shift = torch.ones_like(mx, dtype=torch.bool) if kb == 0 else ((mx > 8.0) if rule == "lazy" else torch.zeros_like(mx, dtype=torch.bool))
                delta = torch.where(shift, mx, torch.zeros_like(mx))
                alpha = torch.exp2(-delta)
                m = m + delta
                p = torch.exp2(s - m)
            l = l * alpha
            if defect != "no_rescale":
                O = O * alpha
            pr = p.to(dt).float()
            if defect == "flush_p" and dt == torch.float16:
                pr = torch.where(pr.abs() < 2.0 ** -14, torch.zeros_like(pr), pr)
            O = O + pr @ vp[sl]
            l = l + (pr if denom_rounded else p).sum(dim=1, keepdim=True)
            if defect == "o16":
                O = O.to(dt).float()
        return O, l

    rows = torch.arange(n)
    if form == "spec":
        O, l = walk(rows, "spec")
        again = ~(torch.isfinite(l[:, 0]) & torch.isfinite(O).all(dim=1))
        if bool(again.any()):
            O2, l2 = walk(rows[again], "lazy")
            O[again], l[again] = O2, l2
    else:
        O, l = walk(rows, form)
    return (O * (1.0 / l)).to(dt)


# ------------------------------------------------------------------------------------------------- input families
def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def make_inputs(family, dt, n, nk, dh, scale, seed=0):
    """``q [n, dh]``, ``k, v [nk, dh]`` of type ``dt`` (one sample, one head; callers stack them)."""
    q, k, v = _randn((n, dh), 3 * seed + 1), _randn((nk, dh), 3 * seed + 2), _randn((nk, dh), 3 * seed + 3)
    if family == "normal":
        pass
    elif family == "peaked":                       # logit std > 10, row maxima that keep rising along the key walk
        q = q * 6.0
        k = k * torch.linspace(0.5, 3.5, nk).reshape(nk, 1)
    elif family == "late_spike":                   # one key near the end dominates: the reference rises in the last block
        k[max(nk - 3, 0)] *= 12.0
    elif family == "dominant":                     # one key in block 0 takes the row; the rest sit ~18 base-2 units below it
        k = 0.25 * k
        q = 0.25 * q + 1.5
        k[min(5, nk - 1)] = 12.5 / (scale * dh * 1.5)
    elif family in ("over_soft", "over_hard"):     # a late key 14.5 / 22 base-2 units above block 0's maximum, for every query:
        k = 0.05 * k                               # the speculative pass's fp16 P reaches 2^14.5 (finite) / overflows (second pass)
        q = 0.05 * q + 1.5
        gap = 14.75 if family == "over_soft" else 22.25
        k[nk - 2] = gap / LOG2E / (scale * dh * 1.5)
    else:
        raise ValueError(family)
    return q.to(dt), k.to(dt), v.to(dt)


def base2_gap_to_median(q, k, scale):
    """Median over queries of (row maximum - row median) of the scores, in base-2 units."""
    s = (q.double() @ k.double().T) * scale * LOG2E
    return float((s.max(dim=1).values - s.median(dim=1).values).median())


def late_key_excess(q, k, scale, key):
    """Per query: score of ``key`` minus the maximum over the first key block, base-2 units (what the speculative pass's P reaches)."""
    s = (q.double() @ k.double().T) * scale * LOG2E
    return s[:, key] - s[:, :KVB].max(dim=1).values
