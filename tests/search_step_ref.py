"""A plain float64 restatement of ONE label step of the device beam search (espnet_amd/csrc/search.hip), independent of
the kernels: numpy, loops, no vectorised cleverness.  It reads exactly what a device step reads and returns everything a
device step writes, so a test can hold each kernel of the step against it.

  params  dict: B, W, V, S, NC, Lmax, T (frame stride), eos, blank, sos, w_dec, w_ctc, w_len, w_lm, use_end_detect, end_cap
  state   dict of numpy arrays, named after EmSearchBuffers (`r` = the buffer of parity i, `anc` likewise):
            alive (n), done (B), tok / parent (Lmax, n), anc (n, Lmax), run_score / run_sdec / run_sctc / run_slen /
            run_slm / s_prev (n), r (n, T, 2), xlens / maxlens / minlens (B), end_count (B), end_pos / end_slot /
            end_forced / end_score / end_sdec / end_sctc / end_slen / end_slm (B, end_cap), best_all (B),
            best_by_len (B, Lmax + 2)
  ctc_lpT (V, B, T) CTC log-probs, transposed as the device holds them
  dec_logp / lm_logp (n, V) the full scorers' log-prob rows (None when the scorer is absent)

The rules restated (reference line numbers as in search.hip's header):
  weighted full score  w_dec*dec + w_len*1 + w_lm*lm, in that order          batch_beam_search.py:289-290
  pre-beam             the S largest, by value descending, token id ascending :291-302 (tie order: the device's contract)
  candidate slots      0..S-1 = the pre-beam, slot S = <eos> (always scored); -inf ("dup") if <eos> is in the pre-beam.
                       All-vocabulary mode (S == V): slot s = token s
  log psi              logsumexp_t(phi[t-1] + x[t]) (+) r[start-1, 0], blank -> LOGZERO, eos -> logaddexp(r[xlen-1])
                                                                              ctc_prefix_score.py:135-144, 166-190
  total                weighted + w_ctc*(psi - s_prev) + running score        batch_beam_search.py:303-314
  selection            per utterance the W largest totals, by value descending, flat index (k*NC + slot) ascending
  new rows             tree, ancestors, running sums, s_prev = psi, r chain   :317-357, scorers/ctc.py:54-62,
                                                                              ctc_prefix_score.py:158-164
  ended list           <eos> or forced at maxlen-1, in row order; end_detect  :359-423, e2e_asr_common.py:14-44
"""
import copy
import math

import numpy as np

LOGZERO = -10000000000.0  # ctc_prefix_score.py:34
D_END = -10.0             # log(1 * exp(-10)), e2e_asr_common.py:14
NEG = -np.inf


def logaddexp(a, b):
    m = max(a, b)
    if m == NEG:
        return NEG
    return m + math.log(math.exp(a - m) + math.exp(b - m))


def logsumexp(xs):
    m = max(xs)
    if m == NEG:
        return NEG
    return m + math.log(math.fsum(math.exp(x - m) for x in xs))


def initial_state(p, xlens, maxlens, minlens, ctc_lpT):
    """What em_search_init leaves (search_init_rows_kernel / search_init_utt_kernel): row 0 of every utterance alive with
    score 0, <sos> at position 0, every ancestor entry the row itself, r = (LOGZERO, cumsum of blank log-probs)."""
    B, W, Lmax, T, cap = p["B"], p["W"], p["Lmax"], p["T"], p["end_cap"]
    n = B * W
    st = dict(alive=np.zeros(n, np.int64), done=np.zeros(B, np.int64), tok=np.full((Lmax, n), -1, np.int64),
              parent=np.full((Lmax, n), -1, np.int64), anc=np.tile(np.arange(n)[:, None], (1, Lmax)),
              run_score=np.full(n, NEG), s_prev=np.zeros(n), r=np.full((n, T, 2), LOGZERO),
              xlens=np.asarray(xlens, np.int64), maxlens=np.asarray(maxlens, np.int64),
              minlens=np.asarray(minlens, np.int64), end_count=np.zeros(B, np.int64),
              end_pos=np.zeros((B, cap), np.int64), end_slot=np.zeros((B, cap), np.int64),
              end_forced=np.zeros((B, cap), np.int64), best_all=np.full(B, NEG), best_by_len=np.full((B, Lmax + 2), NEG))
    for k in ("run_sdec", "run_sctc", "run_slen", "run_slm"):
        st[k] = np.zeros(n)
    for k in ("end_score", "end_sdec", "end_sctc", "end_slen", "end_slm"):
        st[k] = np.zeros((B, cap))
    st["tok"][0, :] = p["sos"]
    for b in range(B):
        st["alive"][b * W] = 1
        st["run_score"][b * W] = 0.0
        if p["w_ctc"] != 0:
            cum = 0.0
            for t in range(T):
                cum += float(ctc_lpT[p["blank"], b, t])
                st["r"][b * W, t, 1] = cum
    return st


def weighted_full(p, dec_logp, lm_logp, r):
    """Weighted sum of the full scorers for row r, scorer order decoder, length_bonus, lm."""
    w = np.zeros(p["V"])
    if p["w_dec"] != 0:
        w = w + p["w_dec"] * np.asarray(dec_logp[r], np.float64)
    if p["w_len"] != 0:
        w = w + p["w_len"] * 1.0
    if p["w_lm"] != 0:
        w = w + p["w_lm"] * np.asarray(lm_logp[r], np.float64)
    return w


def prebeam(w, S):
    """Token ids of the S largest weighted scores: value descending, id ascending."""
    return sorted(range(len(w)), key=lambda v: (-w[v], v))[:S]


def phi(st, r, t, same):
    rn, rb = float(st["r"][r, t, 0]), float(st["r"][r, t, 1])
    return rb if same else logaddexp(rn, rb)


def log_psi(p, st, i, ctc_lpT, r, tk):
    b = r // p["W"]
    xlen = int(st["xlens"][b])
    if tk == p["blank"] and p["eos"] != p["blank"]:
        return LOGZERO
    if tk == p["eos"]:
        return logaddexp(float(st["r"][r, xlen - 1, 0]), float(st["r"][r, xlen - 1, 1]))
    same = tk == int(st["tok"][i, r])
    start = max(i, 1)
    terms = [float(ctc_lpT[tk, b, 0]) if i == 0 else LOGZERO]  # r[start-1, 0] of the extended prefix
    for t in range(start, xlen):
        terms.append(phi(st, r, t - 1, same) + float(ctc_lpT[tk, b, t]))
    return logsumexp(terms)


def r_chain(p, st, i, ctc_lpT, r, tk):
    """Forward variables (r^n, r^b) of prefix(r) + tk over frames [max(i,1)-1, xlen): {t: (rn, rb)}."""
    b = r // p["W"]
    xlen = int(st["xlens"][b])
    same = tk == int(st["tok"][i, r])
    start = max(i, 1)
    out = {}
    if start - 1 >= xlen:
        return out
    rn, rb = (float(ctc_lpT[tk, b, 0]) if i == 0 else LOGZERO), LOGZERO
    out[start - 1] = (rn, rb)
    for t in range(start, xlen):
        nn = logaddexp(rn, phi(st, r, t - 1, same)) + float(ctc_lpT[tk, b, t])
        nb = logaddexp(rn, rb) + float(ctc_lpT[p["blank"], b, t])
        rn, rb = nn, nb
        out[t] = (rn, rb)
    return out


def total_of(p, st, i, ctc_lpT, r, tk, full):
    """(psi, total) of extending row r by token tk whose weighted full score is `full`."""
    psi, tot = 0.0, full
    if p["w_ctc"] != 0:
        psi = log_psi(p, st, i, ctc_lpT, r, tk)
        tot = tot + p["w_ctc"] * (psi - float(st["s_prev"][r]))
    return psi, tot + float(st["run_score"][r])


def candidates(p, st, i, ctc_lpT, dec_logp, lm_logp):
    """Per row: weighted (n, V), cand_tok / cand_full / cand_psi / cand_total (n, NC).  Rows that are not alive, or whose
    utterance is done, carry total -inf in every slot."""
    n, V, S, NC, W = p["B"] * p["W"], p["V"], p["S"], p["NC"], p["W"]
    out = dict(weighted=np.full((n, V), np.nan), cand_tok=np.full((n, NC), -1, np.int64), cand_full=np.full((n, NC), np.nan),
               cand_psi=np.full((n, NC), np.nan), cand_total=np.full((n, NC), NEG), dup=np.zeros((n, NC), bool))
    for r in range(n):
        if not st["alive"][r] or st["done"][r // W]:
            continue
        w = weighted_full(p, dec_logp, lm_logp, r)
        out["weighted"][r] = w
        if S >= V:
            toks = list(range(V))
        else:
            toks = prebeam(w, S) + [p["eos"]]
        for s, tk in enumerate(toks):
            out["cand_tok"][r, s] = tk
            out["cand_full"][r, s] = w[tk]
            if S < V and s == S and tk in toks[:S]:  # <eos> already among the pre-beam: that slot carries it
                out["dup"][r, s] = True
                continue
            out["cand_psi"][r, s], out["cand_total"][r, s] = total_of(p, st, i, ctc_lpT, r, tk, w[tk])
    return out


def select(p, cand_total):
    """sel_idx (n): per utterance the W largest totals by (value descending, flat index ascending); -1 where fewer than W
    finite totals exist."""
    B, W, NC = p["B"], p["W"], p["NC"]
    sel = np.full(B * W, -1, np.int64)
    for b in range(B):
        flat = np.asarray(cand_total[b * W:(b + 1) * W]).reshape(-1)
        order = sorted((j for j in range(W * NC) if flat[j] > NEG), key=lambda j: (-flat[j], j))
        for k, j in enumerate(order[:W]):
            sel[b * W + k] = j
    return sel


def apply_selection(p, st, i, ctc_lpT, dec_logp, lm_logp, sel_idx, cand_tok):
    """The post-step state (update_kernel / tail_kernel + ctc_state_kernel) for the selection `sel_idx` over the candidate
    tokens `cand_tok`: every float is recomputed here in float64 from the pre-step state.  Returns (new state, written)
    where written[rnew] = frames of r the step produced for that row."""
    B, W, NC, Lmax, cap = p["B"], p["W"], p["NC"], p["Lmax"], p["end_cap"]
    new = copy.deepcopy(st)
    written = {}
    for b in range(B):
        was_done = bool(st["done"][b])
        maxlen, minlen = int(st["maxlens"][b]), int(st["minlens"][b])
        rows = []
        for k in range(W):
            rnew = b * W + k
            sel = -1 if was_done else int(sel_idx[rnew])
            rec = dict(valid=sel >= 0, end=False, score=NEG, sdec=0.0, sctc=0.0, slen=0.0, slm=0.0, sprev=0.0)
            if rec["valid"]:
                pk, s = divmod(sel, NC)
                prow = b * W + pk
                tk = int(cand_tok[prow, s])
                w = weighted_full(p, dec_logp, lm_logp, prow)
                psi, rec["score"] = total_of(p, st, i, ctc_lpT, prow, tk, w[tk])
                if p["w_dec"] != 0:
                    rec["sdec"] = float(st["run_sdec"][prow]) + float(dec_logp[prow][tk])
                if p["w_len"] != 0:
                    rec["slen"] = float(st["run_slen"][prow]) + 1.0
                if p["w_lm"] != 0:
                    rec["slm"] = float(st["run_slm"][prow]) + float(lm_logp[prow][tk])
                if p["w_ctc"] != 0:
                    rec["sctc"] = float(st["run_sctc"][prow]) + (psi - float(st["s_prev"][prow]))
                    rec["sprev"] = psi  # select_state: s = log_psi[i, new_id]
                rec.update(prow=prow, tk=tk, end=(tk == p["eos"] or i == maxlen - 1))
                new["anc"][rnew, :i + 1] = st["anc"][prow, :i + 1]
                if i + 1 < Lmax:
                    new["anc"][rnew, i + 1] = rnew
                new["tok"][i + 1, rnew] = tk
                new["parent"][i + 1, rnew] = prow
                if p["w_ctc"] != 0 and not rec["end"]:
                    chain = r_chain(p, st, i, ctc_lpT, prow, tk)
                    for t, v in chain.items():
                        new["r"][rnew, t] = v
                    written[rnew] = sorted(chain)
            alive = rec["valid"] and not rec["end"]
            new["alive"][rnew] = int(alive)
            new["run_score"][rnew] = rec["score"] if alive else NEG
            new["run_sdec"][rnew], new["run_sctc"][rnew] = rec["sdec"], rec["sctc"]
            new["run_slen"][rnew], new["run_slm"][rnew] = rec["slen"], rec["slm"]
            new["s_prev"][rnew] = rec["sprev"]
            rows.append(rec)
        if was_done:
            continue
        cnt, n_alive = int(st["end_count"][b]), 0
        for k, rec in enumerate(rows):  # the ended list, in row order
            if not rec["valid"]:
                continue
            if not rec["end"]:
                n_alive += 1
                continue
            if i < minlen:
                continue
            forced = int(i == maxlen - 1)
            ylen = i + 2 + forced
            if cnt < cap:
                new["end_pos"][b, cnt], new["end_slot"][b, cnt], new["end_forced"][b, cnt] = i + 1, b * W + k, forced
                new["end_score"][b, cnt], new["end_sdec"][b, cnt] = rec["score"], rec["sdec"]
                new["end_sctc"][b, cnt], new["end_slen"][b, cnt], new["end_slm"][b, cnt] = rec["sctc"], rec["slen"], rec["slm"]
                cnt += 1
            new["best_all"][b] = max(new["best_all"][b], rec["score"])
            new["best_by_len"][b, ylen] = max(new["best_by_len"][b, ylen], rec["score"])
        new["end_count"][b] = cnt
        done = n_alive == 0
        if not done and p["use_end_detect"] and cnt > 0:
            count = 0
            for m in range(3):
                if i - m < 0:
                    continue
                v = new["best_by_len"][b, i - m]
                if v > NEG and v - new["best_all"][b] < D_END:
                    count += 1
            done = count == 3
        if done:
            new["done"][b] = 1
    return new, written


def step(p, st, i, ctc_lpT, dec_logp, lm_logp):
    """One whole label step on the restatement's own decisions: (candidates dict + sel_idx, new state, written)."""
    c = candidates(p, st, i, ctc_lpT, dec_logp, lm_logp)
    c["sel_idx"] = select(p, c["cand_total"])
    new, written = apply_selection(p, st, i, ctc_lpT, dec_logp, lm_logp, c["sel_idx"], c["cand_tok"])
    return c, new, written


def prefix_of(st, i, r):
    """Tokens <sos> .. position i of row r (what the decoder's self-attention reads through `anc`)."""
    return [int(st["tok"][j, st["anc"][r, j]]) for j in range(i + 1)]


def collect(p, st):
    """The ended hypotheses of every utterance, best first, as BatchBeamSearch._collect rebuilds them."""
    out = []
    for b in range(p["B"]):
        hyps = []
        for e in range(int(st["end_count"][b])):
            pos, cur = int(st["end_pos"][b, e]), int(st["end_slot"][b, e])
            ys = []
            for j in range(pos, -1, -1):
                ys.append(int(st["tok"][j, cur]))
                cur = int(st["parent"][j, cur])
            ys.reverse()
            if st["end_forced"][b, e]:
                ys.append(p["eos"])
            hyps.append(dict(yseq=ys, score=float(st["end_score"][b, e]),
                             scores=dict(decoder=float(st["end_sdec"][b, e]), ctc=float(st["end_sctc"][b, e]),
                                         length_bonus=float(st["end_slen"][b, e]), lm=float(st["end_slm"][b, e]))))
        hyps.sort(key=lambda h: -h["score"])
        out.append(hyps)
    return out


# ---- the restatement driven from <sos> to the end, the full scorers fed from the oracle's (float32, promoted) ----------
def params_for(B, W, V, T, olens, ctc_weight, penalty=0.0, lm_weight=0.0, maxlenratio=0.0, minlenratio=0.0,
               pre_beam_ratio=1.5):
    """Parameters and length bounds as BatchBeamSearch._search_run derives them (beam_search.py:105-119, 414-429)."""
    maxlens, minlens = [], []
    for tb in olens:
        ml = tb if maxlenratio == 0 else (-int(maxlenratio) if maxlenratio < 0 else max(1, int(maxlenratio * tb)))
        maxlens.append(ml)
        minlens.append(-int(minlenratio) if minlenratio < 0 else int(minlenratio * tb))
    lcap = max(max(maxlens), T if maxlenratio == 0 else 0)
    S = int(pre_beam_ratio * W)
    if not (ctc_weight != 1.0 and S < V and ctc_weight != 0.0):
        S = V
    p = dict(B=B, W=W, V=V, T=T, S=S, NC=S + 1 if S < V else V, Lmax=lcap + 2, end_cap=W * (lcap + 1), sos=V - 1,
             eos=V - 1, blank=0, use_end_detect=int(maxlenratio == 0.0), w_dec=1.0 - ctc_weight, w_ctc=ctc_weight,
             w_len=penalty, w_lm=lm_weight)
    return p, maxlens, minlens


def run_search(sd, enc, heads, num_blocks, beam, ctc_weight, penalty=0.0, maxlenratio=0.0, minlenratio=0.0,
               lm_weight=0.0, lm_conf=None, observer=None):
    """ONE utterance searched by the restatement alone.  enc (T, d).  Returns (n-best, params, largest |log quantity|)."""
    import torch
    import torch.nn.functional as F

    from oracle import beam_search as ob

    T = enc.size(0)
    V = sd["ctc.ctc_lo.weight"].size(0)
    p, maxlens, minlens = params_for(1, beam, V, T, [T], ctc_weight, penalty, lm_weight if lm_conf else 0.0,
                                     maxlenratio, minlenratio)
    with torch.no_grad():
        lp = F.log_softmax(F.linear(enc, sd["ctc.ctc_lo.weight"], sd["ctc.ctc_lo.bias"]), dim=-1)
    ctc_lpT = lp.double().numpy().T[:, None, :].copy()  # (V, 1, T)
    dec = ob.DecoderOracle(sd, enc, heads, num_blocks, maxlens[0]) if p["w_dec"] != 0 else None
    lm = None
    if p["w_lm"] != 0:
        lm = ob.TransformerLMOracle(sd, lm_conf["head"], lm_conf["layer"], lm_conf.get("pos_enc") is not None, maxlens[0])
    memo_d, memo_l = {}, {}

    def scorer_rows(st, i):
        n = p["W"]
        dl = np.zeros((n, V)) if dec is not None else None
        ll = np.zeros((n, V)) if lm is not None else None
        for r in range(n):
            if not st["alive"][r]:
                continue
            pre = tuple(prefix_of(st, i, r))
            with torch.no_grad():
                if dec is not None:
                    if pre not in memo_d:
                        cache = memo_d[pre[:-1]][1] if len(pre) > 1 else dec.init_cache()
                        memo_d[pre] = dec.step(torch.tensor([pre[-1]]), len(pre) - 1, cache)
                    dl[r] = memo_d[pre][0][0].double().numpy()
                if lm is not None:
                    if pre not in memo_l:
                        cache = memo_l[pre[:-1]][1] if len(pre) > 1 else lm.init_cache()
                        memo_l[pre] = lm.step(torch.tensor([list(pre)]), cache)
                    ll[r] = memo_l[pre][0][0].double().numpy()
        return dl, ll

    st = initial_state(p, [T], maxlens, minlens, ctc_lpT)
    big = 0.0
    for i in range(maxlens[0]):
        if st["done"][0]:
            break
        dl, ll = scorer_rows(st, i)
        c, new, _ = step(p, st, i, ctc_lpT, dl, ll)
        if observer is not None:
            observer(i, st, c, new)
        fin = np.concatenate([c["cand_psi"][np.isfinite(c["cand_psi"])], c["cand_total"][np.isfinite(c["cand_total"])]])
        fin = fin[np.abs(fin) < 1e8]  # (LOGZERO terms are no magnitudes of the search)
        big = max(big, float(np.abs(fin).max()) if fin.size else 0.0)
        st = new
    return collect(p, st)[0], p, big
