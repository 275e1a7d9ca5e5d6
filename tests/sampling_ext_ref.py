"""Test helper: the float64 restatement of lmi_decode_sample_ex's kept set (leopard_amd/csrc/sample.h) — HF's warper chain after top-p:
min_p, typical_p, epsilon_cutoff, eta_cutoff — with the margin of a case (how close, relatively, any token comes to any threshold), the
shared case list, and a kernel driver that collects many draws.  Shared by tests/test_sampling_warpers_hf_pin.py (pins this file to
transformers), tests/test_emu_sampling_ext.py (emulator) and tests/test_gpu_sampling_ext.py (MI355X)."""
import math

import numpy as np
import torch

from tests.row_kernels_ref import HEAD, gapped_row
from tests.sampling_ref import kept_set

MIN_MARGIN = 1e-4                 # fp32 arithmetic moves a value by about 1e-6: a case's inputs keep every token this far from every threshold


def params(T=1.0, k=0, p=1.0, min_p=0.0, typ=1.0, eps=0.0, eta=0.0) -> dict:
    return dict(T=T, k=k, p=p, min_p=min_p, typ=typ, eps=eps, eta=eta)


def kept_set_ext(row: torch.Tensor, vocab: int, T=1.0, k=0, p=1.0, min_p=0.0, typ=1.0, eps=0.0, eta=0.0, suppress=()):
    """(indices that can be drawn, score descending and lower index first on ties; the case's margin; notes).  The margin is the
    smallest relative distance of a token's quantity from the threshold it is compared with, over the four warpers (inf: none is on); the
    top token of ``min_p = 1.0`` (w = exp(0) = 1 exactly, kept anyway) is excluded.  notes: what happened on the way — ``top_removed``
    (typical_p dropped the top token), ``typ_group`` / ``eps_group`` / ``eta_group`` (the size of the tie group of scores at the boundary:
    the last band kept by typical_p, the lowest-probability tokens kept by epsilon / eta)."""
    s = (row[:vocab].float().cpu() / torch.tensor(T, dtype=torch.float32)).double().numpy()          # the kernel's fp32 division
    S = np.array(kept_set(row, vocab, T, k, p, suppress), dtype=np.int64)                         # S0: top-k and top-p
    margin, notes = math.inf, {}
    if len(S) == 0:
        return [], margin, notes
    f32 = lambda v: float(np.float32(v))                                                          # the kernel's parameters are fp32
    d = s - s[S].max()                                                # (the top of S0 is the top of the allowed ids)
    w = np.exp(d)

    def rel(values, thr):
        return float(np.min(np.abs(np.asarray(values) / thr - 1.0))) if len(values) else math.inf

    if min_p and min_p > 0:
        m = f32(min_p)
        margin = min(margin, rel([x for x in w[S] if not (m == 1.0 and x == 1.0)], m))
        S = S[w[S] >= m]
    if typ < 1.0:
        t = f32(typ)
        Z = w[S].sum()
        a = math.log(Z) - d[S]
        H = float((w[S] / Z * a).sum())
        sh = np.abs(a - H)
        order = np.argsort(sh, kind="stable")
        cum = np.cumsum(w[S][order]) / Z
        # groups of equal sh (equal scores) reach or miss t together: the cumulative mass at the end of each group decides
        ends = np.nonzero(np.append(sh[order][1:] != sh[order][:-1], True))[0]
        reached = np.nonzero(cum[ends] >= t)[0]
        last = ends[reached[0]] if len(reached) else len(order) - 1
        c = sh[order][last]
        margin = min(margin, rel(cum[ends[:-1]], t))                  # (the last group's mass is 1: "never reached" cannot be close)
        if c > 0:
            margin = min(margin, rel(sh[sh != c], c))
        top = d[S].max()
        keep = sh <= c
        notes["top_removed"] = bool(not keep[d[S] == top].any())
        notes["typ_group"] = int((sh == c).sum())
        S = S[keep]
    for name, val in (("eps", eps), ("eta", eta)):
        if not val or val <= 0:
            continue
        e = f32(val)
        Z = w[S].sum()
        pr = w[S] / Z
        if name == "eta":
            H = float((pr * (math.log(Z) - d[S])).sum())
            e = min(e, math.sqrt(e) * math.exp(-H))
        margin = min(margin, rel(pr, e))
        keep = (pr >= e) | (d[S] == d[S].max())
        low = d[S][keep].min()
        notes[name + "_group"] = int((d[S] == low).sum())
        S = S[keep]
    S = S[np.lexsort((S, -s[S]))]
    return [int(i) for i in S], margin, notes


# ---- the shared cases -----------------------------------------------------------------------------------------------------------------------
# on gapped_row(V, HEAD): each warper alone, stacked on top-k and top-p, all four together, the four edge values
GAPPED_CASES = [
    params(min_p=0.1), params(min_p=0.3), params(T=0.7, min_p=0.05),
    params(typ=0.5), params(typ=0.9), params(typ=0.2),
    params(eps=0.05), params(eps=0.02),
    params(eta=0.05), params(eta=0.3),
    params(k=8, p=0.9, min_p=0.08), params(k=8, p=0.9, typ=0.8), params(k=10, p=0.95, eps=0.03), params(k=8, p=0.9, eta=0.1),
    params(T=1.0, k=10, p=0.95, min_p=0.02, typ=0.9, eps=0.02, eta=0.03),
    params(min_p=1.0), params(typ=1e-6), params(eps=0.99), params(eta=0.99),
]
# on the broad row: typical_p can remove the top token here
BROAD_CASES = [
    params(typ=0.2), params(typ=0.5), params(typ=0.3, min_p=0.02), params(eta=0.6),
    params(T=0.8, k=40, p=0.98, min_p=0.03, typ=0.6, eps=0.005, eta=0.01),
]
# on the tie row: whole tie groups at the typical boundary and as the lowest kept by epsilon / eta
TIE_CASES = [params(typ=0.6), params(eps=0.04), params(eta=0.2), params(k=7, p=0.9, typ=0.7, eps=0.02)]
# one stacked set per vocabulary size for the chi-square of the draws
CHI2_CASE = params(T=0.9, k=10, p=0.97, min_p=0.03, typ=0.95, eps=0.01, eta=0.02)


def broad_row() -> torch.Tensor:
    return torch.randn(256, generator=torch.Generator().manual_seed(11)) * 1.5


def tie_row(V: int = 512) -> torch.Tensor:
    """Every score level is a tie group of two or three tokens at scattered indices."""
    row = torch.full((V,), -200.0)
    levels = {3.0: [17, 300], 2.4: [5, 130, 411], 1.9: [64, 65], 1.0: [2, 250, 499], 0.3: [100, 101], -0.6: [7, 8, 9]}
    for v, where in levels.items():
        row[where] = v
    return row


def kept_probs_ext(row: torch.Tensor, kept: list, T: float) -> np.ndarray:
    s = (row[kept].float().cpu() / torch.tensor(T, dtype=torch.float32)).double().numpy()
    w = np.exp(s - s.max())
    return w / w.sum()


def ext_tensors(n: int, c: dict, dev):
    """(temperature, top_k, top_p, {min_p, typical_p, epsilon_cutoff, eta_cutoff}) device tensors of n rows of the case c."""
    f = lambda v: torch.full((n,), float(v), dtype=torch.float32, device=dev)
    return f(c["T"]), torch.full((n,), int(c["k"]), dtype=torch.int32, device=dev), f(c["p"]), dict(
        min_p=f(c["min_p"]), typical_p=f(c["typ"]), epsilon_cutoff=f(c["eps"]), eta_cutoff=f(c["eta"]))


def draw_many_ext(ops, row: torch.Tensor, vocab: int, c: dict, n_rows: int, n_steps: int, seed0: int = 1, suppress=None,
                  logits: torch.Tensor = None) -> np.ndarray:
    """n_rows x n_steps draws from one logits row through decode_sample_ex: n_rows copies in one launch (seeds seed0..), the kernel
    advancing step itself (tests/sampling_ref.draw_many).  ``logits``: the [n_rows, >= vocab] rows to use instead of copies of ``row``."""
    if logits is None:
        logits = row.reshape(1, -1).expand(n_rows, -1).contiguous()
    dev = logits.device
    temp, k, p, ext = ext_tensors(n_rows, c, dev)
    seed = torch.arange(seed0, seed0 + n_rows, dtype=torch.int64, device=dev)
    step = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    tok = torch.zeros(n_rows, dtype=torch.int64, device=dev)
    pos = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    out = []
    for _ in range(n_steps):
        ops.decode_sample_ex(logits, vocab, temp, k, p, seed, step, tok, pos, suppress=suppress, **ext)
        out.append(tok.cpu().numpy().copy())
    return np.concatenate(out)


def steps_to_see_all(probs: np.ndarray, n_rows: int, at_most: int) -> int:
    """Launches of n_rows draws after which every kept token is expected more than 8 times (asserted to fit ``at_most``)."""
    n = int(math.ceil(8.5 / (float(probs.min()) * n_rows)))
    assert n <= at_most, ("a kept token is too unlikely to show up in the draws of this case", float(probs.min()), n, at_most)
    return max(n, 2)


def check_kept_set_equals_draws(ops, row: torch.Tensor, vocab: int, c: dict, n_rows: int, at_most: int, suppress=None, logits=None):
    """The set of the draws of case c is the float64 kept set, whose margin is asserted first; returns (kept, notes)."""
    sup = () if suppress is None else [int(j) for j in suppress.tolist()]
    kept, margin, notes = kept_set_ext(row, vocab, suppress=sup, **c)
    assert margin >= MIN_MARGIN, (c, margin)
    probs = kept_probs_ext(row, kept, c["T"])
    steps = steps_to_see_all(probs, n_rows, at_most)
    draws = draw_many_ext(ops, row, vocab, c, n_rows, steps, suppress=suppress, logits=logits)
    assert set(draws.tolist()) == set(kept), (c, sorted(set(draws.tolist()) ^ set(kept)))
    return kept, notes


# ---- the kernel-level checks both device files run (ops: the emulator's or the MI355X's; dev: "cpu" or the device) ---------------------------
def unaligned_rows(row: torch.Tensor, n_rows: int, dev) -> torch.Tensor:
    """n_rows copies of ``row`` (its length + 1 a multiple of 4) as a [n_rows, ld] view none of whose row pointers is 16-byte aligned."""
    ld = row.numel() + 1
    assert ld % 4 == 0
    buf = torch.zeros(1 + n_rows * ld, dtype=torch.float32)
    view = buf[1:].view(n_rows, ld)
    view[:, :row.numel()] = row
    view[:, row.numel():] = 100.0                                     # behind the vocabulary: must never be drawn
    out = buf.to(dev)[1:].view(n_rows, ld)
    assert all((out[r].data_ptr() % 16) != 0 for r in range(n_rows))
    return out


def check_special_rows(ops, dev):
    """One allowed token; a suppressed id that the filters would keep; rows of NaN and -inf only give token 0."""
    c = params(k=10, p=0.95, min_p=0.02, typ=0.9, eps=0.02, eta=0.03)
    V = 1000
    one = torch.full((1024,), float("-inf"))
    one[1024 - 24:] = 100.0
    one[421] = -3.0
    assert set(draw_many_ext(ops, one.to(dev), V, c, 8, 2).tolist()) == {421}
    row = gapped_row(V, HEAD, seed=1, ld=1024)
    plain, _, _ = kept_set_ext(row, V, **c)
    sup = torch.tensor([plain[1]], dtype=torch.int64)
    kept, _ = check_kept_set_equals_draws(ops, row.to(dev), V, c, 64, 16, suppress=sup.to(dev))
    assert plain[1] not in kept and plain[0] in kept
    bad = torch.full((3, 1024), float("nan"))
    bad[1] = float("-inf")
    bad[2, ::2] = float("-inf")
    bad[:, V:] = 100.0
    temp, k, p, ext = ext_tensors(3, c, dev)
    tok = torch.full((3,), 7, dtype=torch.int64, device=dev)
    ops.decode_sample_ex(bad.to(dev), V, temp, k, p, torch.arange(3, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int32, device=dev),
                         tok, torch.zeros(3, dtype=torch.int32, device=dev), **ext)
    assert tok.tolist() == [0, 0, 0]


def check_chi_square(ops, dev, V: int, n_rows: int, n_steps: int):
    from tests.sampling_ref import chi2_ok
    row = gapped_row(V, HEAD, seed=3)
    kept, margin, _ = kept_set_ext(row, V, **CHI2_CASE)
    assert margin >= MIN_MARGIN and len(kept) >= 4
    draws = draw_many_ext(ops, row.to(dev), V, CHI2_CASE, n_rows, n_steps, seed0=1000)
    assert set(draws.tolist()) <= set(kept)
    ok, stat, crit = chi2_ok(draws, kept, kept_probs_ext(row, kept, CHI2_CASE["T"]))
    assert ok, (V, stat, crit)


def _state(n, dev, seed0=5, step0=0):
    return dict(seed=torch.arange(seed0, seed0 + n, dtype=torch.int64, device=dev), step=torch.full((n,), step0, dtype=torch.int32, device=dev),
                tok=torch.zeros(n, dtype=torch.int64, device=dev), pos=torch.zeros(n, dtype=torch.int32, device=dev))


def check_all_off_equals_decode_sample(ops, dev, V: int):
    """With all four off — as arrays of "off" values and as null arrays — decode_sample_ex returns decode_sample's tokens and state."""
    g = torch.Generator().manual_seed(V)
    n = 6
    logits = (torch.randn(n, V, generator=g) * 2.0).to(dev)
    for T, k, p in ((1.0, 0, 1.0), (0.8, 20, 0.9), (1.3, 0, 0.7), (1.0, 5, 1.0)):
        c = params(T=T, k=k, p=p)
        temp, kk, pp, ext = ext_tensors(n, c, dev)
        for seed0 in (1, 1 << 40):
            a, b, z = _state(n, dev, seed0), _state(n, dev, seed0), _state(n, dev, seed0)
            for _ in range(3):
                ops.decode_sample(logits, V, temp, kk, pp, a["seed"], a["step"], a["tok"], a["pos"])
                ops.decode_sample_ex(logits, V, temp, kk, pp, b["seed"], b["step"], b["tok"], b["pos"], **ext)
                ops.decode_sample_ex(logits, V, temp, kk, pp, z["seed"], z["step"], z["tok"], z["pos"])
                for key in ("tok", "step", "pos"):
                    assert torch.equal(a[key], b[key]) and torch.equal(a[key], z[key]), (T, k, p, seed0, key)


def check_rows_are_independent(ops, dev, V: int):
    """Per-row parameters differ within one launch (row 0 plain, row 1 min_p, row 2 typical_p, ...): each row's token is that of its solo
    launch, in another slot of another batch size, over several steps."""
    g = torch.Generator().manual_seed(V + 1)
    cases = [params(), params(min_p=0.2), params(typ=0.4), params(eps=0.01), params(eta=0.05), params(k=30, p=0.9, min_p=0.05, typ=0.8, eps=0.01, eta=0.02),
             params(T=0.7, typ=0.6, eta=0.1)]
    n = len(cases)
    logits = (torch.randn(n, V, generator=g) * 2.0).to(dev)
    cat = lambda ts: torch.cat(ts)
    per = [ext_tensors(1, c, dev) for c in cases]
    temp, kk, pp = cat([t[0] for t in per]), cat([t[1] for t in per]), cat([t[2] for t in per])
    ext = {key: cat([t[3][key] for t in per]) for key in per[0][3]}
    for step0 in (0, 3):
        st = _state(n, dev, seed0=77, step0=step0)
        ops.decode_sample_ex(logits, V, temp, kk, pp, st["seed"], st["step"], st["tok"], st["pos"], **ext)
        for r in range(n):
            solo = _state(1, dev, seed0=77 + r, step0=step0)
            ops.decode_sample_ex(logits[r:r + 1], V, *per[r][:3], solo["seed"], solo["step"], solo["tok"], solo["pos"], **per[r][3])
            assert int(solo["tok"][0]) == int(st["tok"][r]), (V, step0, r, cases[r])
        rev = _state(n, dev, seed0=77, step0=step0)                    # the same rows in the opposite slots
        flip = lambda t: t.flip(0).contiguous()
        rev["seed"] = flip(rev["seed"])
        ops.decode_sample_ex(flip(logits), V, flip(temp), flip(kk), flip(pp), rev["seed"], rev["step"], rev["tok"], rev["pos"],
                             **{key: flip(v) for key, v in ext.items()})
        assert torch.equal(rev["tok"].flip(0), st["tok"]), (V, step0)
