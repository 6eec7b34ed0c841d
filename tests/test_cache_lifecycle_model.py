"""CPU: the life-cycle scripts of tests/cache_lifecycle.py are self-consistent, and they reject the mistakes a stateful cache
layer can make.

(a) every script passes with :class:`ShadowCache` itself as the subject, for every configuration: the script builder, the
    capacity prediction (24, 56, 120 asserted literally by the scripts' ``expect`` steps) and the driver agree;
(b) discrimination: ``ShadowCache(mistake=...)`` as the subject is rejected by the script named for it, by the check named
    for it. A state mistake is caught exactly (bits, lens, capacity, allocation, staging). An output-only mistake must move
    some element by >= 5x the suite's standard tolerance (the convention of tests/test_key_score_model.py); the test prints
    the measured ratio. Measured with this file (mixed f16 128 / int4 bf16 64 / int8 bf16 128)::

        stale_tokens_after_eviction    185x / 27x / 28x   (evict: the decode step after evict_by_scores)
        extend_appends_first           161x / 21x / 21x   (growth: the first appending chunk, S = 9)
        key_scores_prev_T              250x / 31x / 31x   (growth: key_scores after append_from_past)

    (bf16's tolerance is 8x fp16's.) The others are caught exactly: append_lost_on_growth, append_to_old_T_after_eviction,
    scales_not_gathered, pool_tail_scales_off_by_one by the stored bits; v_lens_not_updated by the token counts;
    cap_reset_by_eviction by the capacity; noop_trim_reallocates by the allocation; stage_kept_across_eviction and
    stage_not_copied_on_growth by the incremental view;
(c) the driver's tolerance is ``tests.gpu_harness.within_standard``'s, and every scaled score of the scripts stays below 9
    where no cap is set.
"""
import numpy as np
import pytest

from tests import cache_lifecycle as C

IDS = ["-".join(map(str, c)) for c in C.CONFIGS]


@pytest.mark.parametrize("config", C.CONFIGS, ids=IDS)
@pytest.mark.parametrize("name", C.SCRIPTS)
def test_script_passes_on_the_shadow(name, config):
    mode, dtype, D = config
    report = {}
    C.run_script(C.ShadowCache(C.L, mode, dtype), C.script(name, mode, dtype, D), mode, dtype, name, report)
    assert all(r == 0.0 for r in report.values()), report  # the same model on both sides


def test_scripts_cover_what_they_claim():
    mode, dtype, D = C.CONFIGS[0]
    ops = {name: [op for op, _ in C.script(name, mode, dtype, D)] for name in C.SCRIPTS}
    caps = {name: [kw["cap"] for op, kw in C.script(name, mode, dtype, D) if op == "expect"] for name in C.SCRIPTS}
    assert caps["growth"][:1] == [24] and 56 in caps["growth"] and 120 in caps["growth"] and 312 in caps["growth"]
    assert caps["evict"][:3] == [24, 56, 120] and 136 in caps["evict"]
    assert ops["growth"].count("staging") >= 3 and ops["evict"].count("staging") >= 4
    for need in ("score_evict", "chunk_summarize", "trim", "keep_tokens", "compress_prompt", "extend", "attend"):
        assert need in ops["evict"], need
    assert ops["mid_walk"].count("raises") == 4
    var = [kw for op, kw in C.script("variants", mode, dtype, D) if op in ("attend", "extend")]
    for key in ("window", "kv_start", "softcap", "sinks"):
        assert sum(1 for kw in var if key in kw) >= 6, key
    assert any(kw["append"] and "window" in kw and "sinks" in kw for kw in var)
    assert any(all(k in kw for k in ("window", "kv_start", "softcap", "sinks")) for kw in var)
    # a window that cuts, and a row that sees no stored key
    assert all(kw["window"] < 60 for kw in var if "window" in kw) and all(kw["kv_start"][1] >= 63 for kw in var if "kv_start" in kw)


def test_scores_stay_below_nine_where_no_cap_is_set():
    """the bound attn_mod_cases.SINK_AMP documents for the standard tolerance"""
    for mode, dtype, D in C.CONFIGS:
        for name in C.SCRIPTS:
            sh = C.ShadowCache(C.L, mode, dtype)
            worst = 0.0
            for op, kw in C.script(name, mode, dtype, D):
                kw = {k: v for k, v in kw.items() if k != "noop"}
                if op in ("attend", "extend") and not kw.get("softcap"):
                    T = sh.k.lens[kw["layer"]]
                    kd = sh._kv(kw["layer"], T)[0]
                    q = C.widen(kw["q"], dtype)
                    q = q[:, :, None] if q.ndim == 3 else q
                    keys = [kd]
                    if kw.get("k_new") is not None:
                        kn = C.widen(kw["k_new"], dtype)
                        keys.append(kn[:, :, None] if kn.ndim == 3 else kn)
                    kall = np.repeat(np.concatenate(keys, axis=2), C.HQ // C.HKV, axis=1)
                    worst = max(worst, float(np.abs(np.einsum("bhsd,bhnd->bhsn", q, kall)).max() * D ** -0.5))
                if op == "trim":
                    sh.trim(kw["policy"], **kw["args"])
                elif op == "score_evict":
                    sh.evict_by_scores(sh.key_scores(kw["layer"], kw["q"]), kw["budget"], kw["prefix_len"], kw["recent"], kw["pool"])
                elif op not in ("staging", "expect", "raises", "key_scores"):
                    getattr(sh, op)(**kw)
            assert 7.0 < worst < 9.0, (mode, dtype, D, name, worst)


@pytest.mark.parametrize("config", C.CONFIGS, ids=IDS)
@pytest.mark.parametrize("mistake", sorted(C.MISTAKES))
def test_script_rejects(mistake, config):
    mode, dtype, D = config
    name, check = C.MISTAKES[mistake]
    with pytest.raises(C.StepFailure) as ei:
        C.run_script(C.ShadowCache(C.L, mode, dtype, mistake=mistake), C.script(name, mode, dtype, D), mode, dtype, name)
    e = ei.value
    print(f"{mistake}: {mode} {dtype} {D}: step {e.step} ({e.op}) {e.check}" + (f" {e.ratio:.1f}x the tolerance" if e.ratio else ""))
    assert e.check == check, str(e)
    if check == "output":
        assert e.ratio >= 5.0, str(e)


def test_the_driver_applies_the_standard_tolerance():
    from tests.gpu_harness import within_standard
    rng = np.random.default_rng(0)
    ref = rng.standard_normal((2, 8, 64))
    for dtype in ("f16", "bf16"):
        for scale in (0.2, 0.9, 1.1, 5.0):
            got = ref + scale * C.TOL[dtype] * (np.abs(ref) + np.abs(ref).max()) * rng.choice([-1.0, 1.0], ref.shape)
            r = C.ratio(got, ref, dtype)
            assert abs(r - scale) < 1e-6 * scale
            if r <= 1.0:
                within_standard(got, ref, dtype)
            else:
                with pytest.raises(AssertionError):
                    within_standard(got, ref, dtype)
    assert C.ratio(np.full_like(ref, np.nan), ref, "f16") == float("inf")


def test_the_scripts_refuse_exact_capacities(monkeypatch):
    monkeypatch.setenv("KVQ_STORE_CAP_EXACT", "1")
    mode, dtype, D = C.CONFIGS[0]
    with pytest.raises(AssertionError, match="KVQ_STORE_CAP_EXACT"):
        C.run_script(C.ShadowCache(C.L, mode, dtype), C.script("mid_walk", mode, dtype, D), mode, dtype)
