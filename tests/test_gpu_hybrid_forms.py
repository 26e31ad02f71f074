"""Every form of the hybrid rows' eigen-power step (chain family 6: a row longer than SMCPP_HYB_TH is ONE step P d^s P^-1 inside
k_chain_ss) against the C restatement, at every padded state count and number of eigen keys - tests/hybrid_cases.py holds the table
of forms, the fifteen cases and the builder of their inputs, tests/test_hybrid_forms.py the plan side of it.

Each input is three ragged contigs (about 2 500 rows, about 700, 1) under set_chunking(200) - a dozen chunks, three or four, one -
with parameters from the engine's own preparation.  A case first asserts, on describe()["hybrid"] and the input, that it reached
the form it is written for (form, tables in LDS, cold and hot eigen keys, workgroup wavefronts; chain mode 6; at least two forward
passes; every eigen key with 30 rows above the threshold in the long contig and one in its first and its last chunk), then holds

  * every contig to the restatement with the project's own bars (`_oracle_check(gamma=True)`: LL_TOL, STAT_TOL on the xi sums entry
    by entry and on the per-key gamma sums, check_gamma_columns on every column with the device decode), Q(separate=True) to STAT_TOL;
  * the hybrid route to the dense one on the same input (SMCPP_HYBRID=0, itself held to the restatement): log-likelihood to 1e-8
    relative, xi and gamma sums to 2 STAT_TOL (the bars of test_hybrid_scan_chains_on_unbinned_data);
  * SMCPP_SS_WPC=2 (the eight-wavefront workgroup: one table copy for two wavefronts per SIMD, 18 forward chunks so one workgroup
    holds idle task slots) bit for bit to the default run on every getter: it changes which wavefront runs a chunk, not the arithmetic;
  * SMCPP_HYB_TH = 1 and 40 (6 is the default run) and save_gamma off (the statistics-only route) to the restatement;
  * the padded cases once more on poisoned memory: finite and bit for bit the clean run.

Conditions on every input, from the restatement alone: fewer than 1 % of the columns are within 1e-5 span of a tie (the columns the
decode check leaves out), and giving the rarest eigen key's long rows the most frequent eigen key's key moves the log-likelihood by
more than 100 LL_TOL relative - a kernel that read the wrong key's tables could not pass.  (One eigen key: nothing to swap.)

Every run prints one line that starts with "hybrid forms:" - the form it asserted and its worst value of each measure."""
import numpy as np
import pytest

import hybrid_cases as hc
from conftest import rel_err
from test_gpu_parity import LL_TOL, STAT_TOL
from test_gpu_poison import _clean_and_poisoned, _model_manager, _oracle_check, _oracle_estep, _outputs

pytestmark = pytest.mark.gpu

WPC_CASES = (3, 6, 10, 12, 14)
TH_CASES = (2, 5, 9, 14)
LEAN_CASES = (6, 10, 14)
POISON_CASES = (2, 6, 9, 13)
_IN = {}


def _input(case, r):
    if (case, r) not in _IN:
        _IN[case, r] = hc.case_input(case, r)
    return _IN[case, r]


def _build(inp):
    return _model_manager(inp["n"], inp["contigs"], M=inp["M"], theta=hc.THETA_BP, rho=hc.RHO_BP, chunk=hc.CHUNK_ROWS)


def _oracle(im, contigs):
    ep = im.emission_probs
    keys = im.keys
    Etab = np.array([ep[tuple(k)] for k in keys.tolist()])
    return [_oracle_estep(im.pi, im.transition, keys, Etab, c, True) for c in contigs]


def _held_to_restatement(im, inp, save_gamma, label):
    """The project's bars (asserted by _oracle_check and on Q), and the worst value of each measure, printed."""
    contigs = inp["contigs"]
    os_ = _oracle(im, contigs)
    lls, xs, gss = im.logliks(), im.xisums, im.gamma_sums
    w = {"ll": max(abs(lls[c] - o["loglik"]) / max(1.0, abs(o["loglik"])) for c, o in enumerate(os_)),
         "xisum": max(rel_err(xs[c], o["xisum"]) for c, o in enumerate(os_)),
         "gamma_sums": max(np.max(np.abs(gss[c][k] - v)) / max(np.abs(v).max(), 1e-300) for c, o in enumerate(os_) for k, v in o["gamma_sums"].items())}
    q, qo = np.array(im.Q(separate=True)), np.sum([o["q"] for o in os_], axis=0)
    w["q"] = float(np.max(np.abs(q - qo) / np.maximum(np.abs(qo), 1e-12)))
    if save_gamma:
        gams = im.gammas
        w["gamma"] = max(float(np.max(np.max(np.abs(gams[c][:, 1:] - o["gamma"][:, 1:]), axis=0) / contigs[c][:, 0])) for c, o in enumerate(os_))
    hyb = im.describe()["hybrid"]
    form = "not hybrid (dense family %d)" % im.chain_mode() if hyb is None else \
        "%s, %d tables in LDS, cold %s, hot %d, %d wavefronts, threshold %d, %d emission slots" % (
            hyb["form"], hyb["tables_in_lds"], hyb["cold_eigen_keys"], hyb["hot_eigen_key"], hyb["workgroup_wavefronts"], hyb["threshold"],
            hyb["emission_slots_in_lds"])
    print("hybrid forms: case %d.%d M %d Ke %d %s: %s | %s" % (inp["case"], inp["rotation"], inp["M"], inp["Ke"], label, form,
                                                            ", ".join("%s %.2e" % kv for kv in w.items())))
    _oracle_check(contigs, gamma=save_gamma, oracle_gamma=True)(im)
    assert w["q"] <= STAT_TOL, (label, q, qo)
    return w


def _reached(im, inp, th=hc.TH[0], wavefronts=4):
    """What a case relies on, from describe() and the input."""
    d = im.describe()
    hyb, plan = d["hybrid"], d["plan"]
    assert plan["states_padded"] == inp["Mp"] and plan["eigen_keys"] == inp["Ke"]
    assert im.last_timing()["fwd_passes"] >= 2
    if inp["case"] == 15:                         # five eigen keys: the boundary falls back to the dense chains
        assert hyb is None and im.chain_mode() == 2 and not plan["hybrid_rows"]
        return hyb
    assert im.chain_mode() == 6 and plan["hybrid_rows"]
    assert hyb["form"] == inp["form"] and hyb["tables_in_lds"] == inp["tables_in_lds"] and hyb["eigen_keys"] == inp["Ke"]
    assert hyb["threshold"] == th and hyb["workgroup_wavefronts"] == wavefronts and hyb["hot_eigen_key"] == inp["hot"]
    # the cold keys are the least frequent ones among the rows above the threshold (at SMCPP_HYB_TH's other values as well)
    assert hyb["cold_eigen_keys"] == inp["cold"]
    chunks = im.chunks()
    mine = chunks[chunks[:, 0] == 0]
    assert len(mine) >= 12 and 3 <= int(np.sum(chunks[:, 0] == 1)) <= 4 and int(np.sum(chunks[:, 0] == 2)) == 1
    long_ = inp["contigs"][0]
    for k in inp["eigen_keys"]:
        rows = hc.long_rows(long_, k, th) + 1                        # (the engine's rows: 1-based, a chunk owns r0 + 1 .. r1)
        assert len(rows) >= 30
        for r0, r1 in (mine[0, 1:3], mine[-1, 1:3]):
            assert np.any((rows > r0) & (rows <= r1)), (k, r0, r1)
        for c in inp["contigs"][:2]:                                 # a row on each side of the threshold (at 1: every span-2 row is a step)
            spans = c[np.all(c[:, 1:] == np.array(k), axis=1), 0]
            assert th == 1 or (th in spans and th + 1 in spans)
            assert hc.LONGEST in spans
    return hyb


def _run(inp, engine_opt, env, save_gamma=True):
    for k, v in env.items():
        engine_opt(k, v)
    im = _build(inp)
    im.save_gamma = save_gamma
    out = _outputs(im, save_gamma)
    for k in env:
        engine_opt(k, None)
    return im, out


def _input_conditions(im, inp):
    os_ = _oracle(im, inp["contigs"])
    if inp["M"] > 1:
        weak = cols = 0
        for c, o in zip(inp["contigs"], os_):
            top2 = np.sort(o["gamma"], axis=0)[-2:]
            weak += int(np.sum((top2[1] - top2[0]) <= 1e-5 * np.concatenate([[1.0], c[:, 0].astype(float)])))
            cols += o["gamma"].shape[1]
        assert weak < 0.01 * cols, (weak, cols)
    if inp["Ke"] > 1:
        ll = sum(o["loglik"] for o in os_)
        swapped = hc.with_key_swapped(inp["contigs"], inp["rarest"], inp["most"])
        assert sum(len(hc.long_rows(c, inp["rarest"], hc.TH[0])) for c in swapped) == 0
        ll2 = sum(o["loglik"] for o in _oracle(im, swapped))
        assert abs(ll2 - ll) > 100 * LL_TOL * abs(ll), (ll, ll2)


@pytest.mark.parametrize("case,r", hc.INPUTS)
def test_every_form_against_the_restatement(case, r, engine_opt):
    inp = _input(case, r)
    im, out = _run(inp, engine_opt, {})
    hyb = _reached(im, inp)
    _input_conditions(im, inp)
    if case == 12:
        # more keys than emission slots beside the tables: the ALLLDS = false instantiation.  A key's slot is its rank by rows
        # (build_layout): the two eigen keys hold most rows and sit in LDS, the span-1 keys fill the rest of it and the global path
        assert not hyb["all_keys_in_lds"]
        nlds, K = hyb["emission_slots_in_lds"], im.describe()["plan"]["keys"]
        assert K == len(inp["keys"]) >= 62 and K > nlds == 48
        rows = np.concatenate([c[:, 1:] for c in inp["contigs"]])
        count = {k: int(np.sum(np.all(rows == np.array(k), axis=1))) for k in inp["keys"]}
        slot = {k: s for s, k in enumerate(sorted(sorted(inp["keys"]), key=lambda k: -count[k]))}
        assert all(slot[k] < nlds for k in inp["eigen_keys"])
        others = [slot[k] for k in inp["keys"] if k not in inp["eigen_keys"]]
        assert min(others) < nlds <= max(others) and sum(s >= nlds for s in others) == K - nlds
    elif hyb is not None:
        assert hyb["all_keys_in_lds"]
    _held_to_restatement(im, inp, True, "default")
    del im
    if case != 15:
        # the dense route on the same input: itself to the restatement, then the two routes to each other
        dm, dense = _run(inp, engine_opt, {"SMCPP_HYBRID": "0"})
        assert dm.chain_mode() == 2 and dm.describe()["hybrid"] is None
        _held_to_restatement(dm, inp, True, "dense route")
        del dm
        ll = abs(out["loglik"].sum() - dense["loglik"].sum()) / abs(dense["loglik"].sum())
        xi = max(rel_err(a, b) for a, b in zip(out["xisum"], dense["xisum"]))
        gs = np.max(np.abs(out["gamma_sums"] - dense["gamma_sums"]) / np.maximum(np.abs(dense["gamma_sums"]).max(axis=1, keepdims=True), 1e-300))
        print("hybrid forms: case %d.%d hybrid against dense route: ll %.2e, xisum %.2e, gamma_sums %.2e" % (case, r, ll, xi, gs))
        assert np.array_equal(out["gamma_keys"], dense["gamma_keys"])
        assert ll <= 1e-8 and xi <= 2 * STAT_TOL and gs <= 2 * STAT_TOL
    if r:
        return                                                        # (the switch variants: on a case's first weighting)
    if case in WPC_CASES:
        wm, wide = _run(inp, engine_opt, {"SMCPP_SS_WPC": "2"})
        _reached(wm, inp, wavefronts=8)
        nf = len(wm.chunks())
        assert nf % 8 != 0, nf                                        # idle task slots in one workgroup
        print("hybrid forms: case %d.%d eight-wavefront workgroup, %d forward chunks: bit for bit" % (case, r, nf))
        del wm
        for k, v in out.items():
            assert np.array_equal(wide[k], v), f"SMCPP_SS_WPC=2 differs from the default run in {k}: largest {np.max(np.abs(wide[k] - v)):.3e}"
    if case in TH_CASES:
        for th in (1, 40):
            tm, _ = _run(inp, engine_opt, {"SMCPP_HYB_TH": str(th)})
            _reached(tm, inp, th=th)
            _held_to_restatement(tm, inp, True, "threshold %d" % th)
            del tm
    if case in LEAN_CASES:
        lm, _ = _run(inp, engine_opt, {}, save_gamma=False)
        _reached(lm, inp)
        _held_to_restatement(lm, inp, False, "save_gamma off")
        del lm


@pytest.mark.parametrize("case", POISON_CASES)
def test_padded_forms_on_poisoned_memory(case, engine_opt):
    """M < Mp on several chunks: the eigenvalue loads are guarded by the state count, table rows clamped, padded table entries zero -
    nothing of it may come from memory the E-step did not write."""
    inp = _input(case, 0)
    assert inp["M"] < inp["Mp"]

    def check(im):
        _reached(im, inp)
        _held_to_restatement(im, inp, True, "clean run of the poison pair")
    _clean_and_poisoned(engine_opt, lambda: _build(inp), check, True)
