"""The calls of tests/test_engine_calls_cpu.py: every public method of HipEngine accepted at least once (each optional operand present
and absent), and every `raise ValueError` / `raise RuntimeError` of the engine's host side reached by a call with exactly one thing
wrong.  B = 2 with unequal rows, a handful of frames and tokens, S = 64.  Each case gets fresh operands and a fresh stand-in engine.

    python -m tests.helpers.engine_cases <commit>     rewrites tests/golden/engine_calls.txt.gz from the engine.py in the tree"""
import gzip
import os
import sys
import types
import warnings
from unittest import mock

import numpy as np
import torch

from .engine_standin import BYTES, make_engine, record

NS = types.SimpleNamespace
B, N, P, R, S, T, CN, L, H, DH = 2, 5, 4, 3, 64, 6, 7, 12, 8, 120
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "engine_calls.txt.gz")


def f32(*s):
    return torch.zeros(*s)


def i32(*s):
    return torch.zeros(*s, dtype=torch.int32)


def i64(*s):
    return torch.zeros(*s, dtype=torch.int64)


def u8(*s):
    return torch.zeros(*s, dtype=torch.uint8)


def boolean(*s):
    return torch.ones(*s, dtype=torch.bool)


def cache(rows, r, p):
    return {"k_ref": f32(L, rows, H, r, DH), "v_ref": f32(L, rows, H, r, DH), "ref_mask": boolean(rows, r),
            "k_text": f32(L, rows, H, p, DH), "v_text": f32(L, rows, H, p, DH), "ph_mask": boolean(rows, p)}


def operands():
    o = NS()
    o.ref, o.ref_len, o.ids, o.ph_mask = f32(B, R, 64), torch.tensor([3, 2]), torch.ones(B, P, dtype=torch.int64), boolean(B, P)
    o.cache, o.cache3, o.cache0 = cache(B, R, P), cache(3 * B, R, P), cache(B, R, 0)
    o.mask, o.noise, o.x_pin, o.pin = boolean(B, N), f32(4, B, N, 64), f32(B, N, 64), boolean(B, N)
    o.x_t, o.t, o.rope = f32(B, N, 64), f32(B), f32(N, 64)
    o.mass, o.spans, o.path_score = f32(B, N, P), i32(B, P, 2), f32(B)
    o.x, o.x6, o.logp, o.tokens = f32(B, N, 64), f32(B, 6, 64), f32(B, T, CN), i32(B, P)
    o.emb, o.refe, o.total, o.keep = f32(4, 8), f32(2, 8), f32(B), boolean(B, N)
    o.total_new, o.counts, o.feat_cur, o.feat_new, o.x_new = f32(B), i32(B, 2), i32(B, 4), i32(B, 4), f32(B, N, 64)
    o.spans_new, o.mass_new = i32(B, P, 2), f32(B, N, P)
    o.latents, o.pool, o.dpool, o.mpool = f32(B, 3, 64), u8(3, BYTES), u8(3, BYTES), u8(3, BYTES)
    o.audio, o.fade, o.out, o.out16 = f32(B, 1, S), f32(16), f32(200), torch.zeros(200, dtype=torch.int16)
    o.seg, o.gain, o.jstate = i64(B, 2), f32(B), i64(2)
    o.chunk, o.dtable, o.audio2 = f32(S), i64(4), f32(B, S)
    o.k1, o.v1, o.k2, o.v2 = f32(L, 1, H, 3, DH), f32(L, 1, H, 3, DH), f32(L, 1, H, 2, DH), f32(L, 1, H, 2, DH)
    return o


ns, ns6, ts, p0, p1, lens, offsets = [5, 3], [6, 4], [6, 4], [0, 1], [4, 3], [40, 24], [0, 50]
takes = NS(weights=(1.0, 0.5, 0.25, 2.0), tau_token=0.125, tau_frame=0.25)
repair = NS(tau_token=0.375, max_span=10, margin=2)
ep = NS(kernel_params=lambda: {"W": 16, "rel_pow": 0.001, "floor_pow": 1e-8, "min_run": 2, "lead": 1, "tail": 3, "target_rms": 0.1,
                               "peak_limit": 0.9, "max_gain": 4.0})
tap = NS(layers=[1, 3], heads=None, steps=[0, -1])


def meta(t):
    return torch.empty(t.shape, dtype=t.dtype, device="meta")


def strided(t):
    """same dtype and shape, not contiguous"""
    return torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype)[..., ::2]


def misaligned(t):
    """same dtype and shape, contiguous, 8 bytes off a 16-byte boundary"""
    raw = torch.zeros(t.numel() * t.element_size() + 8, dtype=torch.uint8)
    return raw[8:].view(t.dtype).view(t.shape)


def ep_with(**kw):
    return NS(kernel_params=lambda: dict(ep.kernel_params(), **kw))


def no_gpu(lib):
    from smalltts_amd.engine import HipEngine
    with mock.patch.object(torch.cuda, "is_available", lambda: False):
        return HipEngine(0)


def construct(lib):
    from smalltts_amd.engine import HipEngine
    return HipEngine(0, "bf16x3,attn=f16")


def single_stream(lib):
    with mock.patch.dict(os.environ, {"SMTTS_SINGLE_STREAM": "1"}):
        eng = make_engine(lib)
        eng._first = eng.set_dual_stream(True)
    del lib.calls[:]
    return eng


def quiet(fn):
    def run(e, o):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return fn(e, o)
    return run


def prepared(setup):
    """an engine on which `setup` has run, its calls dropped"""
    def build(lib):
        eng = make_engine(lib)
        setup(eng)
        del lib.calls[:]
        return eng
    return build


profiling = dict(env_engine=prepared(lambda e: e.profile(True)))
slotted = dict(env_engine=prepared(lambda e: e.use_workspace("a")))


def attention(e, o, hook, **kw):
    q, w = f32(B, N, 4 * 2 * 8), f32(8)
    return getattr(e, hook)(q, w, w, 1e-6, f32(N, 4), 4, 2, 8, **kw)


KV = dict(k_ref=f32(B, 2, R, 8), v_ref=f32(B, 2, R, 8), k_text=f32(B, 2, P, 8), v_text=f32(B, 2, P, 8), mask_self=boolean(B, N),
          mask_ref=boolean(B, R), mask_text=boolean(B, P))

# (title, fn(engine, operands), stand-in options)
CASES = [
    # ---- construction and plumbing
    ("HipEngine() preset and site override", lambda e, o: e.precision, dict(env_engine=construct)),
    ("refused: HipEngine() without a GPU", lambda e, o: None, dict(env_engine=no_gpu)),
    ("refused: HipEngine() smtts_create fails", lambda e, o: None, dict(env_engine=construct, fail=["smtts_create"])),
    ("close twice", lambda e, o: (e.close(), e.close(), e.h), {}),
    ("refused: a call the library fails", lambda e, o: e.randn(8, 3), dict(fail=["smtts_randn"])),
    ("use_workspace slot then sample", lambda e, o: (e.use_workspace("a"), e.sample(o.cache, o.mask), e._ws is None, sorted(e._ws_named)), {}),
    ("refused: use_workspace while profiling", lambda e, o: e.use_workspace("a"), profiling),
    ("use_workspace None while profiling", lambda e, o: e.use_workspace(None), profiling),
    ("release_workspaces", lambda e, o: (e.randn(4, 1), e.release_workspaces(), e._ws_named), slotted),
    ("set_dual_stream first call", lambda e, o: (e.set_dual_stream(False), e.set_dual_stream(True), e.dual_stream), {}),
    ("set_dual_stream first call under SMTTS_SINGLE_STREAM=1", lambda e, o: (e._first, e.set_dual_stream(False)), dict(env_engine=single_stream)),
    ("set_tuning", lambda e, o: (e.set_tuning("throughput"), e.set_tuning("latency"), e.tuning), {}),
    ("set_ln_fold", lambda e, o: (e.set_ln_fold(False), e.set_ln_fold(True), e.ln_fold), {}),
    ("set_precision preset", lambda e, o: (e.set_precision("bf16"), e.precision), {}),
    ("set_precision with overrides", lambda e, o: e.set_precision("f16,codec_ffn=bf16x3, codec_conv = f16x2"), {}),
    ("refused: set_precision f16x2 as a preset", lambda e, o: e.set_precision("f16x2"), {}),
    ("saturations", lambda e, o: (e.saturations(), e.saturations(reset=False)), {}),
    ("saturations_now", lambda e, o: e.saturations_now(), {}),
    ("check_fp16_range clean", lambda e, o: (e.check_fp16_range("x"), e.check_fp16_range(in_flight=True)), {}),
    ("check_fp16_range demotes codec_ffn and attn, set_precision keeps them",
     quiet(lambda e, o: (e.check_fp16_range("x"), e.check_fp16_range("x"), e.set_precision("bf16"), e.precision_in_force())), dict(saturated=[4, 7])),
    ("precision_in_force", lambda e, o: e.precision_in_force(), {}),
    # ---- weights
    ("set_codec_spec", lambda e, o: e.set_codec_spec(__import__("smalltts_amd.weights").weights.CodecSpec(n_filters=8, dec_depths=(1,) * 7)), {}),
    ("set_tensor torch fp32", lambda e, o: e.set_tensor("a.w", o.ref), {}),
    ("set_tensor numpy fp64 scalar", lambda e, o: e.set_tensor("a.s", np.float64(2.0)), {}),
    ("load_state_dict", lambda e, o: e.load_state_dict({"a.w": o.ref, "a.b": np.zeros((3,), np.float32)}), {}),
    ("load_synthetic asr only", lambda e, o: e.load_synthetic(3, parts=("asr",)), {}),
    ("get_tensor", lambda e, o: e.get_tensor("a.w", (2, 3)), {}),
    ("finalize", lambda e, o: e.finalize(), {}),
    ("finalize drops demotions", quiet(lambda e, o: (e.check_fp16_range(), e.finalize(), e.precision_in_force())), dict(saturated=[0])),
    ("has", lambda e, o: (e.has("dit"), e.has("sv")), {}),
    # ---- the DiT
    ("cond_encode", lambda e, o: e.cond_encode(o.ref, o.ref_len, o.ids, o.ph_mask), {}),
    ("cond_encode debug", lambda e, o: e.cond_encode(o.ref, o.ref_len, o.ids, o.ph_mask, debug=True), {}),
    ("cond_encode converts", lambda e, o: e.cond_encode(o.ref.numpy(), o.ref_len.int(), o.ids.int(), o.ph_mask), {}),
    ("denoise_step", lambda e, o: e.denoise_step(o.x_t, o.mask, o.t, o.cache), {}),
    ("denoise_step rope", lambda e, o: e.denoise_step(o.x_t, o.mask, o.t, o.cache, rope=o.rope), {}),
    ("sample plain", lambda e, o: e.sample(o.cache, o.mask, noise=o.noise, seed=9), {}),
    ("sample align", lambda e, o: e.sample(o.cache, o.mask, noise=o.noise, seed=9, align=True), {}),
    ("sample pinned", lambda e, o: e.sample(o.cache, o.mask, noise=o.noise, seed=9, x_pin=o.x_pin), {}),
    ("sample pinned align", lambda e, o: e.sample(o.cache, o.mask, noise=o.noise, seed=9, x_pin=o.x_pin, align=True), {}),
    ("sample ode no noise steps", lambda e, o: e.sample(o.cache, o.mask, num_steps=3, mode="ode", return_steps=True), {}),
    ("sample cfg", lambda e, o: e.sample(o.cache3, o.mask, cfg=True, s_text=2.5, s_spk=1.25), {}),
    ("sample align selection steps", lambda e, o: e.sample(o.cache, o.mask, align=tap, return_steps=True), {}),
    ("sample align False", lambda e, o: e.sample(o.cache, o.mask, align=False), {}),
    ("sample pinned pin start_step steps align selection",
     lambda e, o: e.sample(o.cache, o.mask, x_pin=o.x_pin, pin=o.pin, start_step=2, return_steps=True, align=tap), {}),
    ("sample pinned misaligned x_pin and noise", lambda e, o: e.sample(o.cache, o.mask, noise=misaligned(o.noise), x_pin=misaligned(o.x_pin)), {}),
    ("sample pinned numpy x_pin", lambda e, o: e.sample(o.cache, o.mask, x_pin=o.x_pin.numpy(), pin=o.pin.numpy()), {}),
    ("refused: sample pinned ode", lambda e, o: e.sample(o.cache, o.mask, mode="ode", x_pin=o.x_pin), {}),
    ("refused: sample start_step 4 of 4", lambda e, o: e.sample(o.cache, o.mask, x_pin=o.x_pin, start_step=4), {}),
    ("refused: sample pin without x_pin", lambda e, o: e.sample(o.cache, o.mask, pin=o.pin), {}),
    ("refused: sample x_pin fp64", lambda e, o: e.sample(o.cache, o.mask, x_pin=o.x_pin.double()), {}),
    ("refused: sample pin not an array", lambda e, o: e.sample(o.cache, o.mask, x_pin=o.x_pin, pin=[1, 0]), {}),
    ("refused: sample pinned align without text keys", lambda e, o: e.sample(o.cache0, o.mask, x_pin=o.x_pin, align=True), {}),
    ("refused: sample align without text keys", lambda e, o: e.sample(o.cache0, o.mask, align=True), {}),
    ("refused: sample align steps out of range", lambda e, o: e.sample(o.cache, o.mask, align=NS(layers=None, heads=None, steps=[4])), {}),
    ("refused: sample align layers out of range", lambda e, o: e.sample(o.cache, o.mask, align=NS(layers=[12], heads=None, steps=None)), {}),
    # ---- alignment and scorers
    ("align_path", lambda e, o: e.align_path(o.mass, ns, p0, p1), {}),
    ("refused: align_path mass fp64", lambda e, o: e.align_path(o.mass.double(), ns, p0, p1), {}),
    ("refused: align_path mass on another device", lambda e, o: e.align_path(meta(o.mass), ns, p0, p1), {}),
    ("refused: align_path N 226", lambda e, o: e.align_path(f32(B, 226, P), ns, p0, p1), {}),
    ("refused: align_path three counts", lambda e, o: e.align_path(o.mass, [5, 3, 1], p0, p1), {}),
    ("asr_logprobs", lambda e, o: e.asr_logprobs(o.x, ns), {}),
    ("asr_logprobs out", lambda e, o: e.asr_logprobs(o.x, ns, out=f32(B, 4 * N, 198)), {}),
    ("sv_embed", lambda e, o: e.sv_embed(o.x6, ns6), {}),
    ("sv_embed out", lambda e, o: e.sv_embed(o.x6, ns6, out=f32(B, 192)), {}),
    ("refused: asr_logprobs x not contiguous", lambda e, o: e.asr_logprobs(strided(o.x), ns), {}),
    ("refused: sv_embed N 5", lambda e, o: e.sv_embed(o.x, ns), {}),
    ("refused: asr_logprobs one count", lambda e, o: e.asr_logprobs(o.x, [5]), {}),
    ("refused: asr_logprobs no recogniser", lambda e, o: e.asr_logprobs(o.x, ns), dict(parts=0)),
    ("refused: sv_embed out shape", lambda e, o: e.sv_embed(o.x6, ns6, out=f32(B, 191)), {}),
    ("sv_cosine", lambda e, o: e.sv_cosine(o.emb, o.refe, K=2), {}),
    ("refused: sv_cosine ref int32", lambda e, o: e.sv_cosine(o.emb, o.refe.int(), K=2), {}),
    ("refused: sv_cosine K 3", lambda e, o: e.sv_cosine(o.emb, o.refe, K=3), {}),
    ("refused: sv_cosine ref rows", lambda e, o: e.sv_cosine(o.emb, o.refe, K=1), {}),
    ("ctc_score", lambda e, o: e.ctc_score(o.logp, ts, o.tokens, p0, p1), {}),
    ("refused: ctc_score logp 2-d", lambda e, o: e.ctc_score(o.logp[0], ts, o.tokens, p0, p1), {}),
    ("refused: ctc_score tokens int64", lambda e, o: e.ctc_score(o.logp, ts, o.tokens.long(), p0, p1), {}),
    ("refused: ctc_score C 1", lambda e, o: e.ctc_score(f32(B, T, 1), ts, o.tokens, p0, p1), {}),
    ("refused: ctc_score one p1", lambda e, o: e.ctc_score(o.logp, ts, o.tokens, p0, [4]), {}),
    ("ctc_align", lambda e, o: e.ctc_align(o.logp, ts, o.tokens, p0, p1), {}),
    ("ctc_align frames", lambda e, o: e.ctc_align(o.logp, ts, o.tokens, p0, p1, frames=True), {}),
    ("refused: ctc_align logp on another device", lambda e, o: e.ctc_align(meta(o.logp), ts, o.tokens, p0, p1), {}),
    ("refused: ctc_align tokens rows", lambda e, o: e.ctc_align(o.logp, ts, i32(3, P), p0, p1), {}),
    ("refused: ctc_align T 1025", lambda e, o: e.ctc_align(f32(B, 1025, CN), ts, o.tokens, p0, p1), {}),
    ("refused: ctc_align one ts", lambda e, o: e.ctc_align(o.logp, [6], o.tokens, p0, p1), {}),
    ("ctc_greedy", lambda e, o: e.ctc_greedy(o.logp, ts), {}),
    ("refused: ctc_greedy logp fp16", lambda e, o: e.ctc_greedy(o.logp.half(), ts), {}),
    ("refused: ctc_greedy T 4097", lambda e, o: e.ctc_greedy(f32(1, 4097, 2), [1]), {}),
    ("refused: ctc_greedy three counts", lambda e, o: e.ctc_greedy(o.logp, [6, 4, 1]), {}),
    # ---- takes and repair
    ("take_scores", lambda e, o: e.take_scores(o.mass, o.spans, o.path_score, ns, p0, p1, takes), {}),
    ("refused: take_scores mass not contiguous", lambda e, o: e.take_scores(strided(o.mass), o.spans, o.path_score, ns, p0, p1, takes), {}),
    ("refused: take_scores P 199", lambda e, o: e.take_scores(f32(B, N, 199), o.spans, o.path_score, ns, p0, p1, takes), {}),
    ("refused: take_scores spans shape", lambda e, o: e.take_scores(o.mass, i32(B, P, 3), o.path_score, ns, p0, p1, takes), {}),
    ("refused: take_scores path_score fp64", lambda e, o: e.take_scores(o.mass, o.spans, o.path_score.double(), ns, p0, p1, takes), {}),
    ("refused: take_scores one p0", lambda e, o: e.take_scores(o.mass, o.spans, o.path_score, ns, [0], p1, takes), {}),
    ("refused: take_scores a negative weight",
     lambda e, o: e.take_scores(o.mass, o.spans, o.path_score, ns, p0, p1, NS(weights=(1, -1, 0, 0), tau_token=0.1, tau_frame=0.1)), {}),
    ("take_select", lambda e, o: e.take_select(o.total, 2, o.x, ns), {}),
    ("take_select spans mass", lambda e, o: e.take_select(o.total, 1, o.x, ns, spans=o.spans, mass=o.mass), {}),
    ("take_select mass only", lambda e, o: e.take_select(o.total, 2, o.x, ns, mass=o.mass), {}),
    ("refused: take_select total 2-d", lambda e, o: e.take_select(f32(B, 1), 2, o.x, ns), {}),
    ("refused: take_select K 3", lambda e, o: e.take_select(o.total, 3, o.x, ns), {}),
    ("refused: take_select x width", lambda e, o: e.take_select(o.total, 2, f32(B, N, 63), ns), {}),
    ("refused: take_select N 226", lambda e, o: e.take_select(o.total, 2, f32(B, 226, 64), ns), {}),
    ("refused: take_select spans fp32", lambda e, o: e.take_select(o.total, 2, o.x, ns, spans=f32(B, P, 2)), {}),
    ("refused: take_select mass frames", lambda e, o: e.take_select(o.total, 2, o.x, ns, mass=f32(B, N + 1, P)), {}),
    ("refused: take_select one count", lambda e, o: e.take_select(o.total, 2, o.x, [5]), {}),
    ("repair_plan", lambda e, o: e.repair_plan(o.mass, o.spans, ns, p0, p1, repair), {}),
    ("repair_plan keep", lambda e, o: e.repair_plan(o.mass, o.spans, ns, p0, p1, repair, keep=o.keep), {}),
    ("repair_plan keep uint8", lambda e, o: e.repair_plan(o.mass, o.spans, ns, p0, p1, repair, keep=u8(B, N)), {}),
    ("refused: repair_plan mass fp64", lambda e, o: e.repair_plan(o.mass.double(), o.spans, ns, p0, p1, repair), {}),
    ("refused: repair_plan N 226", lambda e, o: e.repair_plan(f32(B, 226, P), o.spans, ns, p0, p1, repair), {}),
    ("refused: repair_plan spans on another device", lambda e, o: e.repair_plan(o.mass, meta(o.spans), ns, p0, p1, repair), {}),
    ("refused: repair_plan keep int32", lambda e, o: e.repair_plan(o.mass, o.spans, ns, p0, p1, repair, keep=i32(B, N)), {}),
    ("refused: repair_plan three counts", lambda e, o: e.repair_plan(o.mass, o.spans, [5, 3, 1], p0, p1, repair), {}),
    ("refused: repair_plan margin 33", lambda e, o: e.repair_plan(o.mass, o.spans, ns, p0, p1, NS(tau_token=0.1, max_span=10, margin=33)), {}),
    ("repair_keep", lambda e, o: e.repair_keep(o.total, o.total_new, o.counts, o.feat_cur, o.feat_new, o.x, o.x_new), {}),
    ("repair_keep spans mass",
     lambda e, o: e.repair_keep(o.total, o.total_new, o.counts, o.feat_cur, o.feat_new, o.x, o.x_new, o.spans, o.spans_new, o.mass, o.mass_new), {}),
    ("repair_keep mass only",
     lambda e, o: e.repair_keep(o.total, o.total_new, o.counts, o.feat_cur, o.feat_new, o.x, o.x_new, mass_cur=o.mass, mass_new=o.mass_new), {}),
    ("refused: repair_keep total_cur 2-d", lambda e, o: e.repair_keep(f32(B, 1), o.total_new, o.counts, o.feat_cur, o.feat_new, o.x, o.x_new), {}),
    ("refused: repair_keep total_new rows", lambda e, o: e.repair_keep(o.total, f32(3), o.counts, o.feat_cur, o.feat_new, o.x, o.x_new), {}),
    ("refused: repair_keep counts int64", lambda e, o: e.repair_keep(o.total, o.total_new, o.counts.long(), o.feat_cur, o.feat_new, o.x, o.x_new), {}),
    ("refused: repair_keep x_new frames", lambda e, o: e.repair_keep(o.total, o.total_new, o.counts, o.feat_cur, o.feat_new, o.x, f32(B, N + 1, 64)), {}),
    ("refused: repair_keep spans_new missing",
     lambda e, o: e.repair_keep(o.total, o.total_new, o.counts, o.feat_cur, o.feat_new, o.x, o.x_new, spans_cur=o.spans), {}),
    ("refused: repair_keep N 226",
     lambda e, o: e.repair_keep(o.total, o.total_new, o.counts, o.feat_cur, o.feat_new, f32(B, 226, 64), f32(B, 226, 64)), {}),
    ("refused: repair_keep spans_new not contiguous",
     lambda e, o: e.repair_keep(o.total, o.total_new, o.counts, o.feat_cur, o.feat_new, o.x, o.x_new, o.spans, strided(o.spans_new)), {}),
    ("refused: repair_keep mass_new fp64",
     lambda e, o: e.repair_keep(o.total, o.total_new, o.counts, o.feat_cur, o.feat_new, o.x, o.x_new, mass_cur=o.mass, mass_new=o.mass_new.double()), {}),
    # ---- the codec
    ("hop", lambda e, o: e.hop, {}),
    ("codec_decode", lambda e, o: e.codec_decode(o.latents), {}),
    ("decode_state_bytes", lambda e, o: e.decode_state_bytes, {}),
    ("refused: decode_state_bytes 0", lambda e, o: e.decode_state_bytes, dict(zero=["smtts_decode_state_bytes"])),
    ("decode_state", lambda e, o: e.decode_state(3), {}),
    ("refused: decode_state 0 slots", lambda e, o: e.decode_state(0), {}),
    ("codec_decode_stream", lambda e, o: e.codec_decode_stream(o.latents, o.pool, [2, 0]), {}),
    ("refused: codec_decode_stream latents width", lambda e, o: e.codec_decode_stream(f32(B, 3, 63), o.pool, [2, 0]), {}),
    ("refused: codec_decode_stream state misaligned", lambda e, o: e.codec_decode_stream(o.latents, misaligned(o.pool), [2, 0]), {}),
    ("refused: codec_decode_stream state not a tensor", lambda e, o: e.codec_decode_stream(o.latents, None, [2, 0]), {}),
    ("refused: codec_decode_stream a slot twice", lambda e, o: e.codec_decode_stream(o.latents, o.pool, [2, 2]), {}),
    ("codec_encode", lambda e, o: e.codec_encode(o.audio), {}),
    ("codec_encode cuts to whole hops", lambda e, o: e.codec_encode(f32(B, 1, S + 3)), {}),
    ("codec_encode under one hop", lambda e, o: e.codec_encode(f32(B, 1, 7)), {}),
    ("randn", lambda e, o: e.randn(8, 3, stream_id=2), {}),
    # ---- long form
    ("_upload_i64", lambda e, o: e._upload_i64([[0, 40], [0, 24]]), {}),
    ("voice_expand pairs", lambda e, o: e.voice_expand([(o.k1, o.v1), (o.k2, o.v2)]), {}),
    ("voice_expand objects", lambda e, o: e.voice_expand([NS(k_ref=o.k2, v_ref=o.v2)]), {}),
    ("refused: voice_expand no voices", lambda e, o: e.voice_expand([]), {}),
    ("refused: voice_expand v_ref frames", lambda e, o: e.voice_expand([(o.k1, o.v2)]), {}),
    ("randn_rows", lambda e, o: e.randn_rows([7, -1], ns, 4), {}),
    ("randn_rows n_max", lambda e, o: e.randn_rows([7, 2 ** 63], ns, 2, n_max=8), {}),
    ("refused: randn_rows one seed", lambda e, o: e.randn_rows([7], ns, 4), {}),
    ("stitch", lambda e, o: e.stitch(o.audio, ns, offsets, None, o.out), {}),
    ("stitch fade int16", lambda e, o: e.stitch(o.audio, ns, offsets, o.fade, o.out16), {}),
    ("stitch empty fade", lambda e, o: e.stitch(o.audio, ns, offsets, f32(0), o.out), {}),
    ("refused: stitch a row longer than S", lambda e, o: e.stitch(o.audio, [9, 3], offsets, None, o.out), {}),
    ("refused: stitch out 2-d", lambda e, o: e.stitch(o.audio, ns, offsets, None, f32(2, 100)), {}),
    ("refused: stitch a row behind out", lambda e, o: e.stitch(o.audio, ns, [0, 177], None, o.out), {}),
    ("refused: stitch fade fp64", lambda e, o: e.stitch(o.audio, ns, offsets, o.fade.double(), o.out), {}),
    ("endpoints ns", lambda e, o: e.endpoints(o.audio, ns, ep), {}),
    ("endpoints lens peaks", lambda e, o: e.endpoints(o.audio, None, ep, lens=[64, 0], return_peaks=True), {}),
    ("refused: endpoints audio 2-d", lambda e, o: e.endpoints(o.audio2, ns, ep), {}),
    ("refused: endpoints ns and lens", lambda e, o: e.endpoints(o.audio, ns, ep, lens=lens), {}),
    ("refused: endpoints a length behind S", lambda e, o: e.endpoints(o.audio, None, ep, lens=[65, 0]), {}),
    ("refused: endpoints W 18", lambda e, o: e.endpoints(o.audio, ns, ep_with(W=18)), {}),
    ("stitch_seg", lambda e, o: e.stitch_seg(o.audio, o.seg, None, offsets, None, o.out), {}),
    ("stitch_seg gain fade int16", lambda e, o: e.stitch_seg(o.audio, o.seg, o.gain, offsets, o.fade, o.out16), {}),
    ("stitch_seg empty out", lambda e, o: e.stitch_seg(o.audio, o.seg, None, offsets, None, f32(0)), {}),
    ("refused: stitch_seg one offset", lambda e, o: e.stitch_seg(o.audio, o.seg, None, [0], None, o.out), {}),
    ("refused: stitch_seg seg int32", lambda e, o: e.stitch_seg(o.audio, o.seg.int(), None, offsets, None, o.out), {}),
    ("refused: stitch_seg gain rows", lambda e, o: e.stitch_seg(o.audio, o.seg, f32(3), offsets, None, o.out), {}),
    ("refused: stitch_seg out fp64", lambda e, o: e.stitch_seg(o.audio, o.seg, None, offsets, None, o.out.double()), {}),
    ("refused: stitch_seg an offset behind out", lambda e, o: e.stitch_seg(o.audio, o.seg, None, [0, 201], None, o.out), {}),
    ("refused: stitch_seg fade on another device", lambda e, o: e.stitch_seg(o.audio, o.seg, None, offsets, meta(o.fade), o.out), {}),
    ("join_state", lambda e, o: e.join_state(), {}),
    ("join_stream", lambda e, o: e.join_stream(o.audio, o.seg, None, None, 0, o.jstate, last=False, pcm16=False), {}),
    ("join_stream gain fade gap last pcm16 cap slot",
     lambda e, o: e.join_stream(o.audio, o.seg, o.gain, o.fade, 12, o.jstate, last=True, pcm16=True, cap=100, deliver_slot=2), {}),
    ("refused: join_stream audio 2-d", lambda e, o: e.join_stream(o.audio2, o.seg, None, None, 0, o.jstate, last=False, pcm16=False), {}),
    ("refused: join_stream audio fp64", lambda e, o: e.join_stream(o.audio.double(), o.seg, None, None, 0, o.jstate, last=False, pcm16=False), {}),
    ("refused: join_stream seg not contiguous", lambda e, o: e.join_stream(o.audio, strided(o.seg), None, None, 0, o.jstate, last=False, pcm16=False), {}),
    ("refused: join_stream gain fp64", lambda e, o: e.join_stream(o.audio, o.seg, o.gain.double(), None, 0, o.jstate, last=False, pcm16=False), {}),
    ("refused: join_stream fade not contiguous", lambda e, o: e.join_stream(o.audio, o.seg, None, strided(o.fade), 0, o.jstate, last=False, pcm16=False), {}),
    ("refused: join_stream state int32", lambda e, o: e.join_stream(o.audio, o.seg, None, None, 0, o.jstate.int(), last=False, pcm16=False), {}),
    ("refused: join_stream gap -1", lambda e, o: e.join_stream(o.audio, o.seg, None, None, -1, o.jstate, last=False, pcm16=False), {}),
    ("refused: join_stream cap 0", lambda e, o: e.join_stream(o.audio, o.seg, None, None, 0, o.jstate, last=False, pcm16=False, cap=0), {}),
    # ---- front and back end
    ("resample 1-d 16 kHz", lambda e, o: e.resample(o.chunk, 16_000), {}),
    ("resample 2-d 16 kHz twice, one bank", lambda e, o: (e.resample(o.audio2, 16_000), e.resample(o.audio2, 16_000), len(e._banks)), {}),
    ("resample at the target rate", lambda e, o: e.resample(o.chunk.tolist(), 24_000), {}),
    ("pcm16", lambda e, o: e.pcm16(o.audio), {}),
    # ---- delivery
    ("deliver_bank 24 kHz", lambda e, o: e.deliver_bank(24_000), {}),
    ("deliver_bank 16 kHz zeros 8", lambda e, o: e.deliver_bank(16_000, 8)[1:], {}),
    ("deliver_state", lambda e, o: e.deliver_state(3, 16_000), {}),
    ("deliver_state 24 kHz", lambda e, o: e.deliver_state(3, 24_000), {}),
    ("refused: deliver_state 0 slots", lambda e, o: e.deliver_state(0, 16_000), {}),
    ("refused: deliver_state bytes 0", lambda e, o: e.deliver_state(3, 16_000), dict(zero=["smtts_deliver_state_bytes"])),
    ("deliver whole 24 kHz", lambda e, o: e.deliver(o.audio, lens, 24_000), {}),
    ("deliver whole 24 kHz ignores n_before and last", lambda e, o: e.deliver(o.audio, lens, 24_000, "alaw", n_before=[3, 4], last=False), {}),
    ("deliver whole 16 kHz pcm16", lambda e, o: e.deliver(o.audio, lens, 16_000, "pcm16"), {}),
    ("deliver whole 8 kHz mulaw zeros 8", lambda e, o: e.deliver(o.audio, lens, 8_000, "mulaw", zeros=8), {}),
    ("deliver pooled 16 kHz", lambda e, o: e.deliver(o.audio, lens, 16_000, state=o.dpool, slots=[2, 0], n_before=[7, 9], last=[False, True]), {}),
    ("deliver whole 24 kHz mark", lambda e, o: e.deliver(o.audio, lens, 24_000, mark=(5, 0.02)), {}),
    ("deliver whole 16 kHz mark object", lambda e, o: e.deliver(o.audio, lens, 16_000, mark=NS(key=2 ** 64 - 1, strength=0.5)), {}),
    ("deliver pooled 16 kHz mark mark_state",
     lambda e, o: e.deliver(o.audio, lens, 16_000, state=o.dpool, slots=[2, 0], n_before=[7, 9], last=False, mark=(5, 0.02), mark_state=o.mpool), {}),
    ("deliver 24 kHz mark mark_state", lambda e, o: e.deliver(o.audio, lens, 24_000, slots=[1, 2], n_before=[7, 9], mark=(5, 0.02), mark_state=o.mpool), {}),
    ("refused: deliver mark_state without mark", lambda e, o: e.deliver(o.audio, lens, 24_000, mark_state=o.mpool), {}),
    ("refused: deliver encoding", lambda e, o: e.deliver(o.audio, lens, 24_000, "pcm8"), {}),
    ("refused: deliver audio 2-d", lambda e, o: e.deliver(o.audio2, lens, 24_000), {}),
    ("refused: deliver a length behind S", lambda e, o: e.deliver(o.audio, [65, 0], 24_000), {}),
    ("refused: deliver n_before -1", lambda e, o: e.deliver(o.audio, lens, 24_000, n_before=[-1, 0]), {}),
    ("refused: deliver state at 24 kHz", lambda e, o: e.deliver(o.audio, lens, 24_000, state=o.dpool, slots=[2, 0]), {}),
    ("refused: deliver state width", lambda e, o: e.deliver(o.audio, lens, 16_000, state=u8(3, BYTES - 16), slots=[2, 0]), {}),
    ("refused: deliver slot 3 of 3", lambda e, o: e.deliver(o.audio, lens, 16_000, state=o.dpool, slots=[3, 0]), {}),
    ("refused: deliver slots without state", lambda e, o: e.deliver(o.audio, lens, 16_000, slots=[2, 0]), {}),
    ("refused: deliver n_before without state at 16 kHz", lambda e, o: e.deliver(o.audio, lens, 16_000, n_before=[1, 0]), {}),
    ("refused: deliver mark_state on another device", lambda e, o: e.deliver(o.audio, lens, 24_000, slots=[1, 2], mark=(5, 0.02), mark_state=meta(o.mpool)), {}),
    ("refused: deliver mark_state no slots", lambda e, o: e.deliver(o.audio, lens, 24_000, mark=(5, 0.02), mark_state=o.mpool), {}),
    ("refused: deliver mark key 2^64", lambda e, o: e.deliver(o.audio, lens, 24_000, mark=(2 ** 64, 0.02)), {}),
    ("refused: deliver mark strength 1.5", lambda e, o: e.deliver(o.audio, lens, 24_000, mark=(5, 1.5)), {}),
    ("deliver_from_table 24 kHz", lambda e, o: e.deliver_from_table(o.chunk, o.dtable, 24_000, "pcm16"), {}),
    ("deliver_from_table 16 kHz whole", lambda e, o: e.deliver_from_table(o.chunk, o.dtable, 16_000), {}),
    ("deliver_from_table 16 kHz pooled mark mark_state",
     lambda e, o: e.deliver_from_table(o.chunk, o.dtable, 16_000, "mulaw", state=o.dpool, mark=(5, 0.02), mark_state=o.mpool), {}),
    ("deliver_from_table 24 kHz mark", lambda e, o: e.deliver_from_table(o.chunk, o.dtable, 24_000, mark=(5, 0.02)), {}),
    ("refused: deliver_from_table mark_state without mark", lambda e, o: e.deliver_from_table(o.chunk, o.dtable, 24_000, mark_state=o.mpool), {}),
    ("refused: deliver_from_table encoding", lambda e, o: e.deliver_from_table(o.chunk, o.dtable, 24_000, "pcm8"), {}),
    ("refused: deliver_from_table chunk 2-d", lambda e, o: e.deliver_from_table(o.audio2, o.dtable, 24_000), {}),
    ("refused: deliver_from_table dtable int32", lambda e, o: e.deliver_from_table(o.chunk, o.dtable.int(), 24_000), {}),
    ("refused: deliver_from_table state at 24 kHz", lambda e, o: e.deliver_from_table(o.chunk, o.dtable, 24_000, state=o.dpool), {}),
    ("refused: deliver_from_table state not contiguous", lambda e, o: e.deliver_from_table(o.chunk, o.dtable, 16_000, state=strided(o.dpool)), {}),
    ("refused: deliver_from_table mark_state uint8 1-d", lambda e, o: e.deliver_from_table(o.chunk, o.dtable, 24_000, mark=(5, 0.02), mark_state=u8(BYTES)), {}),
    # ---- watermark
    ("watermark_state", lambda e, o: e.watermark_state(3), {}),
    ("refused: watermark_state 0 slots", lambda e, o: e.watermark_state(0), {}),
    ("watermark", lambda e, o: e.watermark(o.audio, lens, 5), {}),
    ("watermark state", lambda e, o: e.watermark(o.audio, lens, 5, 0.05, state=o.mpool, slots=[2, 0], n_before=[7, 9]), {}),
    ("refused: watermark audio int16", lambda e, o: e.watermark(o.audio.short(), lens, 5), {}),
    ("refused: watermark one length", lambda e, o: e.watermark(o.audio, [40], 5), {}),
    ("refused: watermark n_before -1", lambda e, o: e.watermark(o.audio, lens, 5, n_before=[0, -1]), {}),
    ("refused: watermark state misaligned", lambda e, o: e.watermark(o.audio, lens, 5, state=misaligned(o.mpool), slots=[2, 0]), {}),
    ("refused: watermark slot -1", lambda e, o: e.watermark(o.audio, lens, 5, state=o.mpool, slots=[-1, 0]), {}),
    ("refused: watermark slots without state", lambda e, o: e.watermark(o.audio, lens, 5, slots=[2, 0]), {}),
    ("refused: watermark strength -0.1", lambda e, o: e.watermark(o.audio, lens, 5, -0.1), {}),
    ("watermark_detect", lambda e, o: e.watermark_detect(o.audio2, lens, 5), {}),
    ("watermark_detect offsets u", lambda e, o: e.watermark_detect(o.audio2, lens, 5, o_lo=3, n_off=4, return_u=True), {}),
    ("refused: watermark_detect audio 3-d", lambda e, o: e.watermark_detect(o.audio, lens, 5), {}),
    ("refused: watermark_detect a length behind S", lambda e, o: e.watermark_detect(o.audio2, [65, 0], 5), {}),
    ("refused: watermark_detect key -1", lambda e, o: e.watermark_detect(o.audio2, lens, -1), {}),
    ("refused: watermark_detect n_off 0", lambda e, o: e.watermark_detect(o.audio2, lens, 5, n_off=0), {}),
    ("refused: watermark_detect workspace 0", lambda e, o: e.watermark_detect(o.audio2, lens, 5), dict(zero=["smtts_watermark_detect_workspace_bytes"])),
    # ---- profiling and the rest
    ("profile on tagged shapes off", lambda e, o: (e.profile(True), e.profile(True, tagged=True), e.profile(True, shapes=True), e.profile(False)), {}),
    ("refused: profile with a workspace slot", lambda e, o: e.profile(True), slotted),
    ("profile_report", lambda e, o: e.profile_report(), {}),
    ("alpha_sigma", lambda e, o: e.alpha_sigma(0.5), {}),
    # ---- the hooks
    ("test_gemm", lambda e, o: e.test_gemm(f32(4, 8), f32(6, 8)), {}),
    ("test_gemm bias act split cfg", lambda e, o: e.test_gemm(f32(4, 8), f32(6, 8), bias=f32(6), act="gelu", split=1, cfg=2), {}),
    ("test_gemm3", lambda e, o: e.test_gemm3(f32(4, 8), f32(6, 8)), {}),
    ("test_gemm3 bias act split cfg", lambda e, o: e.test_gemm3(f32(4, 8), f32(6, 8), bias=f32(6), act="mish", split=2, cfg=1), {}),
    ("test_ln_fold", lambda e, o: e.test_ln_fold(f32(4, 6), f32(4, 8), f32(6, 8), f32(4, 6), f32(10, 6), f32(10, 6)), {}),
    ("test_ln_fold every operand",
     lambda e, o: e.test_ln_fold(f32(4, 6), f32(4, 8), f32(6, 8), f32(4, 6), f32(10, 6), f32(10, 6), shift=f32(4, 6), bp=f32(6), gate=f32(4, 6),
                                 row_mask=u8(4), b1=f32(10), b3=f32(10), rms=True, fold=False, precision="bf16x3", eps=1e-5, return_shift=True), {}),
    ("test_codec_stage decoder", lambda e, o: e.test_codec_stage("decoder", 1, 6, f32(B, 3, 4)), {}),
    ("test_codec_stage encoder audio", lambda e, o: e.test_codec_stage(2, 0, 1, f32(B, 16)), {}),
    ("test_dit_stage dit modulation", lambda e, o: e.test_dit_stage("dit", 1, t=o.t), {}),
    ("test_dit_stage dit embed blocks head",
     lambda e, o: e.test_dit_stage("dit", 14, x=o.x, mask=o.mask, l0=1, l1=3, path="fold", twice=True, mod=f32(B, 71040), mod_row0=1, mod_rstride=2,
                                   rope=o.rope, **{k: v for k, v in o.cache.items()}), {}),
    ("test_dit_stage text input blocks", lambda e, o: e.test_dit_stage("text", 3, x=o.ids, mask=o.ph_mask), {}),
    ("test_dit_stage style projection kv", lambda e, o: e.test_dit_stage("style", 12, x=f32(B, R, 512), mask=boolean(B, R), path="unsplit"), {}),
    ("test_scorer_taps sv", lambda e, o: e.test_scorer_taps("sv", f32(B, 7, 64), [7, 6]), {}),
    ("test_scorer_taps asr", lambda e, o: e.test_scorer_taps("asr", f32(B, 3, 64), [3, 1]), {}),
    ("test_swiglu", lambda e, o: e.test_swiglu(f32(4, 8), f32(6, 8), f32(6, 8)), {}),
    ("test_swiglu biases split", lambda e, o: e.test_swiglu(f32(4, 8), f32(6, 8), f32(6, 8), b1=f32(6), b3=f32(6), split=1), {}),
    ("test_attention", lambda e, o: attention(e, o, "test_attention"), {}),
    ("test_attention every operand", lambda e, o: attention(e, o, "test_attention", **KV), {}),
    ("test_attention mfma img", lambda e, o: attention(e, o, "test_attention", mfma="img", **KV), {}),
    ("test_attention mfma img:f16", lambda e, o: attention(e, o, "test_attention", mfma="img:f16"), {}),
    ("test_attn_text_mass", lambda e, o: attention(e, o, "test_attn_text_mass", **KV), {}),
    ("test_attn_text_mass text keys only f16", lambda e, o: attention(e, o, "test_attn_text_mass", k_text=KV["k_text"], v_text=KV["v_text"], fmt="f16"), {}),
    ("refused: test_attn_text_mass without text keys", lambda e, o: attention(e, o, "test_attn_text_mass"), {}),
]


def run():
    """-> (lines, {title: (section lines, stand-in library)})"""
    lines, sections = [], {}
    for title, fn, opts in CASES:
        sec, lib = record(title, fn, operands(), **opts)
        assert title not in sections, title
        sections[title] = (sec, lib)
        lines += sec
    return lines, sections


if __name__ == "__main__":
    with gzip.GzipFile(GOLDEN, "wb", mtime=0) as f:
        f.write(("\n".join([f"# recorded at {sys.argv[1]}"] + run()[0]) + "\n").encode())
