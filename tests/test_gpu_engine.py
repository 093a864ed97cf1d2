"""-m gpu: end-to-end parity of the engine behind GptNeoXOp (through the C ABI) against the oracle and the goldens."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.helpers import load_tiny, quantize_layers, random_model, weight_list_to_layers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    return gpu_helpers


@pytest.fixture(params=["persistent", "launches"], autouse=True)
def decode_path(request, monkeypatch):
    """Every engine test runs twice: with the product defaults (persistent decode-layer kernel for B <= 2, general path with
    the burst GEMMs above) and with the per-stage launches for up to 4 rows (FTCF_PERSIST=0 FTCF_STAGE_MAX_ROWS=4: what one
    row runs under tensor parallelism; the 2..4-row forms stay covered).  The engine reads the variables when it is created."""
    if request.param == "launches" and request.node.get_closest_marker("one_decode_path"):
        pytest.skip("the path this test takes does not depend on the switch: it runs once")
    monkeypatch.setenv("FTCF_PERSIST", "1" if request.param == "persistent" else "0")
    if request.param == "launches":
        monkeypatch.setenv("FTCF_STAGE_MAX_ROWS", "4")
    return request.param


@pytest.fixture(scope="module")
def tiny():
    cfg, w, z = load_tiny()
    layers, glob = weight_list_to_layers(cfg, w)
    return cfg, w, layers, glob, z


# End-to-end bound on |GPU logits - oracle logits| / max|logit|.  The engine reproduces the oracle's elementwise rounding
# points and differs only by fp32 accumulation order and the three documented attention differences:
# measured 1.2e-3 .. 1.3e-3 on the golden model; 5e-3 leaves room for longer contexts and int8, not for a lost rounding point.
LOGIT_FRAC = 5e-3


def _logit_close(got, ref, frac=LOGIT_FRAC):
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() <= frac * scale, (np.abs(got - ref).max() / scale, frac)


def test_tiny_fp16_greedy_is_token_exact_vs_hf_golden_and_oracle(gh, tiny, decode_path):
    cfg, w, layers, glob, z = tiny
    op = gh.make_op(cfg, w)
    r = gh.run_op(op, z["prompt"][None, :], [16], 8, cfg["vocab_size"], top_k=1)
    assert op.stats()["decode_path"] == (1 if decode_path == "persistent" else 0)  # the path under test really ran
    assert r["output_ids"][0, 16:].tolist() == z["hf_tokens"].tolist()
    # directly against HF's fp32 logits (tests/golden/make_golden.py): the fp16 engine's distance from the fp32 model is the
    # half rounding of activations and KV cache -- 1.0e-3 .. 1.5e-3 of max|logit| in the oracle's fp16 mode; bound 4e-3
    hf = z["hf_logits"]
    assert np.abs(r["logits"][:, 0, :] - hf).max() <= 4e-3 * np.abs(hf).max(), np.abs(r["logits"][:, 0, :] - hf).max() / np.abs(hf).max()
    o = orc.Model(dict(cfg, fp16=1), layers, glob).generate(z["prompt"][None, :], [16], 8, return_logits=True)
    assert r["output_ids"].tolist() == o["output_ids"].tolist()
    _logit_close(r["logits"], o["logits"])
    assert r["sequence_lengths"].tolist() == o["sequence_lengths"].tolist()
    np.testing.assert_allclose(r["cum_log_probs"], o["cum_log_probs"], rtol=2e-2, atol=2e-2)


def test_tiny_ragged_batch_and_single_token_prompt(gh, tiny):
    cfg, w, layers, glob, z = tiny
    op = gh.make_op(cfg, w)
    end_id = cfg["end_id"]
    ids = np.full((2, 16), end_id, dtype=np.int32)
    ids[0] = z["prompt"]
    ids[1, :11] = z["prompt_b"]
    r = gh.run_op(op, ids, [16, 11], 8, cfg["vocab_size"], top_k=1)
    assert r["output_ids"][0, :24].tolist() == z["prompt"].tolist() + z["hf_tokens"].tolist()
    assert r["output_ids"][1, :19].tolist() == z["prompt_b"].tolist() + z["hf_tokens_b"].tolist()
    assert r["output_ids"][1, 19:].tolist() == [end_id] * 5
    assert r["sequence_lengths"].tolist() == [24, 24]
    r1 = gh.run_op(op, z["prompt_1"][None, :], [1], 6, cfg["vocab_size"], top_k=1)
    assert r1["output_ids"][0, 1:].tolist() == z["hf_tokens_1"].tolist()


def test_tiny_int8_matches_int8_oracle(gh, tiny):
    cfg, w, layers, glob, z = tiny
    op = gh.make_op(cfg, w, int8_mode=1)
    r = gh.run_op(op, z["prompt"][None, :], [16], 8, cfg["vocab_size"], top_k=1)
    o = orc.Model(dict(cfg, fp16=1, int8_mode=1), quantize_layers(layers), glob).generate(
        z["prompt"][None, :], [16], 8, return_logits=True)
    _logit_close(r["logits"], o["logits"])
    assert r["output_ids"].tolist() == o["output_ids"].tolist()


MID = dict(head_num=8, size_per_head=128, inter_size=4096, num_layer=2, vocab_size=2048, rotary_dim=32, start_id=0,
           end_id=2)


@pytest.mark.parametrize("int8_mode", [0, 1])
@pytest.mark.parametrize("B", [1, 2, 3, 6])
def test_mid_model_fused_and_general_decode_paths(gh, B, int8_mode):
    """H=1024/Dh=128: with the defaults B<=2 runs the persistent layer kernel and B=3, 6 the general path (burst GEMMs);
    in the `launches` variant B<=3 runs the per-stage GEMV launches.  All must follow the oracle.  (The prompt phases of
    B = 3, 6 are 111 / 222 rows: the split-K form of the tiled GEMM.)"""
    _mid_model_follows_the_oracle(gh, B, int8_mode)


@pytest.mark.one_decode_path
@pytest.mark.parametrize("int8_mode", [0, 1])
@pytest.mark.parametrize("max_rows", [16, 64])
def test_mid_model_decode_steps_above_16_rows(gh, monkeypatch, max_rows, int8_mode):
    """20 rows per decode step: the split-K tiled GEMM (default) or, with FTCF_SMALLM_MAX_ROWS=64, the burst GEMM in
    chunks of 16 rows on the two branch streams."""
    monkeypatch.setenv("FTCF_SMALLM_MAX_ROWS", str(max_rows))
    _mid_model_follows_the_oracle(gh, 20, int8_mode, out=6)


@pytest.mark.one_decode_path
@pytest.mark.parametrize("int8_mode", [0, 1])
def test_mid_model_general_path_with_grouped_gemms(gh, monkeypatch, int8_mode):
    """FTCF_DECODE_BRANCHES=0 at TP = 1: six rows on the general path (FTCF_ROWS=0 keeps the rows kernel off it) with the
    independent GEMMs of a layer paired per launch on one stream, where the default is the two-stream branch form."""
    monkeypatch.setenv("FTCF_ROWS", "0")
    monkeypatch.setenv("FTCF_DECODE_BRANCHES", "0")
    op = _mid_model_follows_the_oracle(gh, 6, int8_mode, out=8)
    assert op.stats()["decode_path"] == 2


def _mid_model_follows_the_oracle(gh, B, int8_mode, out=12):
    cfg = MID
    w = random_model(cfg, seed=B + 10 * int8_mode, std=0.04)
    layers, glob = weight_list_to_layers(cfg, w)
    if int8_mode:
        layers = quantize_layers(layers)
    rng = np.random.RandomState(B)
    S = 37
    lens = rng.randint(20, S + 1, size=B).astype(np.int32)
    lens[0] = S
    ids = np.full((B, S), cfg["end_id"], dtype=np.int32)
    for b in range(B):
        ids[b, :lens[b]] = rng.randint(3, cfg["vocab_size"], size=lens[b])
    op = gh.make_op(cfg, w, int8_mode=int8_mode)
    r = gh.run_op(op, ids, lens, out, cfg["vocab_size"], top_k=1)
    o = orc.Model(dict(cfg, fp16=1, int8_mode=int8_mode), layers, glob).generate(ids, lens, out, return_logits=True)
    # compare step by step while the token histories agree (a near-tie may legitimately flip one arg max)
    total_checked = 0
    for b in range(B):
        gen_r = r["output_ids"][b, lens[b]:lens[b] + out]
        gen_o = o["output_ids"][b, lens[b]:lens[b] + out]
        for t in range(out):
            ref = o["logits"][t, b]
            _logit_close(r["logits"][t, b], ref)
            total_checked += 1
            if gen_r[t] != gen_o[t]:
                top2 = np.sort(ref)[-2:]
                assert top2[1] - top2[0] < 2 * LOGIT_FRAC * np.abs(ref).max(), "token flip without a near tie"
                break
    assert total_checked >= B * 2
    return op


def test_sampling_topk_topp_penalties_follow_oracle(gh, tiny):
    cfg, w, layers, glob, z = tiny
    op = gh.make_op(cfg, w)
    B = 3
    # (row 1 used to be the golden prompt reversed: its first step is a tie of 4e-4 of max|logit| between two tokens, which
    # tests the tie, not the sampler)
    ids = np.stack([z["prompt"], np.random.RandomState(1003).randint(3, cfg["vocab_size"], size=16), np.roll(z["prompt"], 3)]).astype(np.int32)
    kw = dict(top_k=[5, 0, 40], top_p=[0.0, 0.7, 0.9], temperature=[0.7, 1.0, 1.3], repetition_penalty=[1.2, 1.0, 1.1],
              random_seed=[11, 22, 33])
    r = gh.run_op(op, ids, [16] * B, 8, cfg["vocab_size"], **kw)
    sp = orc.Sampling(B, **kw)
    o = orc.Model(dict(cfg, fp16=1), layers, glob).generate(ids, [16] * B, 8, sampling=sp, return_logits=True)
    # identical uniforms + (value desc, index asc) ordering on both sides -> identical draws unless fp16-level logit noise
    # moves a cumulative boundary; a row that leaves the oracle's trajectory conditions on another history from there on.
    # Stated per row (round 2 accepted 85 % of all positions): at least two of the three rows are identical to the oracle's
    # from the first to the last token (a cumulative boundary within fp16 noise of the uniform may move one row).  The kernels
    # themselves are checked exactly, on the GPU's own logits, by test_sampling_kernels_reproduce_the_oracle_given_the_same_logits.
    same = [r["output_ids"][b].tolist() == o["output_ids"][b].tolist() for b in range(B)]
    assert sum(same) >= B - 1, (same, r["output_ids"], o["output_ids"])


def test_stop_words_optional_last_tokens_and_callback(gh, tiny):
    cfg, w, layers, glob, z = tiny
    op = gh.make_op(cfg, w)
    toks = z["hf_tokens"].tolist()
    # stop after the 3rd generated token: word list format [B, 2, L] (ids row, cumulative offsets row padded -1)
    stop = np.array([[[toks[1], toks[2]], [2, -1]]], dtype=np.int32)
    events = []
    r = gh.run_op(op, z["prompt"][None, :], [16], 8, cfg["vocab_size"], top_k=1, stop_words=stop,
                  callback=lambda d: events.append(d))
    sp = orc.Sampling(1, stop_words=stop)
    o = orc.Model(dict(cfg, fp16=1), layers, glob).generate(z["prompt"][None, :], [16], 8, sampling=sp)
    assert r["output_ids"].tolist() == o["output_ids"].tolist()
    assert r["output_ids"][0, 16:19].tolist() == toks[:3] and r["sequence_lengths"].tolist() == [19]
    assert [e["last_tokens"][0][0] for e in events] == toks[:3]
    allowed = np.array([[toks[3], toks[5], -1, -1]], dtype=np.int32)
    r2 = gh.run_op(op, z["prompt"][None, :], [16], 4, cfg["vocab_size"], top_k=1, optional_last_tokens=allowed)
    o2 = orc.Model(dict(cfg, fp16=1), layers, glob).generate(
        z["prompt"][None, :], [16], 4, sampling=orc.Sampling(1, optional_last_tokens=allowed))
    assert r2["output_ids"][0, 16] in (toks[3], toks[5])
    assert r2["output_ids"].tolist() == o2["output_ids"].tolist()


@pytest.mark.one_decode_path
@pytest.mark.parametrize("dh", [48, 80, 96, 160, 256])
def test_other_head_sizes_run_the_general_path_against_the_oracle(gh, dh):
    """size_per_head outside {64, 128} (the reference dispatches 32 ... 256, decoder_masked_multihead_attention.cu:29-59): the
    engine takes the general path -- one attention launch per layer, lane groups padded to a power of two -- for one row and
    for a ragged batch, fp16 and int8; tokens and logits against the oracle."""
    cfg = dict(head_num=4, size_per_head=dh, inter_size=4 * 64 * 4, num_layer=2, vocab_size=512, rotary_dim=16, start_id=0,
               end_id=2)
    if (4 * dh) % 64:
        pytest.skip("hidden size must be a multiple of 64")
    for int8_mode in (0, 1):
        w = random_model(cfg, seed=300 + dh, std=0.05)
        layers, glob = weight_list_to_layers(cfg, w)
        lay = quantize_layers(layers) if int8_mode else layers
        rng = np.random.RandomState(dh)
        S, out = 19, 6
        ids = rng.randint(3, cfg["vocab_size"], size=(3, S)).astype(np.int32)
        lens = [S, 11, 4]
        for b, n in enumerate(lens):
            ids[b, n:] = cfg["end_id"]
        op = gh.make_op(cfg, w, int8_mode=int8_mode)
        o = orc.Model(dict(cfg, fp16=1, int8_mode=int8_mode), lay, glob).generate(ids, lens, out, return_logits=True)
        for B in (1, 3):
            r = gh.run_op(op, ids[:B], lens[:B], out, cfg["vocab_size"], top_k=1)
            assert op.stats()["decode_path"] == 2
            for b in range(B):
                for t in range(out):
                    _logit_close(r["logits"][t, b], o["logits"][t, b])
                    if r["output_ids"][b, lens[b] + t] != o["output_ids"][b, lens[b] + t]:
                        top2 = np.sort(o["logits"][t, b])[-2:]
                        assert top2[1] - top2[0] < 2 * LOGIT_FRAC * np.abs(o["logits"][t, b]).max(), "token flip without a near tie"
                        break


def test_engine_is_deterministic_across_calls(gh, tiny):
    cfg, w, layers, glob, z = tiny
    op = gh.make_op(cfg, w, int8_mode=1)
    a = gh.run_op(op, z["prompt"][None, :], [16], 8, cfg["vocab_size"], top_k=1)
    b = gh.run_op(op, z["prompt"][None, :], [16], 8, cfg["vocab_size"], top_k=1)
    assert np.array_equal(a["logits"], b["logits"]) and np.array_equal(a["output_ids"], b["output_ids"])


_VARIANT_REF = {}


@pytest.mark.parametrize("variant", ["grid24", "grid40", "grid32", "grid48", "own0"])
@pytest.mark.parametrize("int8_mode", [0, 1])
def test_persistent_kernel_variants_agree(gh, monkeypatch, decode_path, variant, int8_mode):
    """The persistent decode-layer kernel under other launch shapes: a grid of 24 or 40 workgroups (several runs and attention
    splits per workgroup, other K piece counts) changes the fp32 summation order only, so it stays within the GEMV tolerance of
    the default grid.
    Grids of 32 / 48 workgroups put the out-proj / FFN2 stage into the own-group layout (round 6: whole column groups per
    workgroup -- two of this model's 64, and at 48 workgroups one each plus a third of one of the 16 left over, whose merger
    adds partials published from inside the other pieces' streams); own0 switches that layout off."""
    if decode_path != "persistent":
        pytest.skip("variants of the persistent path only")
    cfg = MID
    w = random_model(cfg, seed=77 + int8_mode, std=0.04)
    rng = np.random.RandomState(5)
    B, S, out = 2, 21, 10
    lens = np.array([S, 13], dtype=np.int32)
    ids = np.full((B, S), cfg["end_id"], dtype=np.int32)
    for b in range(B):
        ids[b, :lens[b]] = rng.randint(3, cfg["vocab_size"], size=lens[b])
    if int8_mode not in _VARIANT_REF:  # (the default launch shape once per weight form: every variant compares against it)
        op = gh.make_op(cfg, w, int8_mode=int8_mode)
        _VARIANT_REF[int8_mode] = gh.run_op(op, ids, lens, out, cfg["vocab_size"], top_k=1)
        assert op.stats()["decode_path"] == 1
        del op
    ref = _VARIANT_REF[int8_mode]
    if variant == "own0":
        monkeypatch.setenv("FTCF_PERSIST_NB", "32")
        monkeypatch.setenv("FTCF_PERSIST_OWN", "0")
    else:
        monkeypatch.setenv("FTCF_PERSIST_NB", variant[4:])
        monkeypatch.setenv("FTCF_PERSIST_OWN", "1")  # (the default, 2, takes the layout only where it measured faster)
    op2 = gh.make_op(cfg, w, int8_mode=int8_mode)
    got = gh.run_op(op2, ids, lens, out, cfg["vocab_size"], top_k=1)
    assert op2.stats()["decode_path"] == 1
    assert op2.stats()["persist_layout"] == (1 if variant in ("grid32", "grid48") else 0)  # (the layout under test really ran)
    for t in range(out):
        for b in range(B):
            _logit_close(got["logits"][t, b], ref["logits"][t, b])
            if got["output_ids"][b, lens[b] + t] != ref["output_ids"][b, lens[b] + t]:
                break


def test_long_sequences_leave_the_single_pass_attention_forms(gh, tiny):
    """4200-token prompt (s_max = 4206): a KV split (16 at most) no longer fits the all-in-registers attention form of the
    per-stage kernels (256 keys at size_per_head 64), which then run the looped form; the persistent kernel takes more keys
    per split.  The first decode step already attends over the whole range; logits follow the oracle on either path."""
    cfg, w, layers, glob, z = tiny
    op = gh.make_op(cfg, w)
    S, out = 4200, 6
    ids = np.random.RandomState(5).randint(3, cfg["vocab_size"], size=(1, S)).astype(np.int32)
    r = gh.run_op(op, ids, [S], out, cfg["vocab_size"], top_k=1)
    o = orc.Model(dict(cfg, fp16=1), layers, glob).generate(ids, [S], out, return_logits=True)
    gen_r, gen_o = r["output_ids"][0, S:], o["output_ids"][0, S:]
    for t in range(out):
        _logit_close(r["logits"][t, 0], o["logits"][t, 0])
        if gen_r[t] != gen_o[t]:
            top2 = np.sort(o["logits"][t, 0])[-2:]
            assert top2[1] - top2[0] < 2 * LOGIT_FRAC * np.abs(o["logits"][t, 0]).max(), "token flip without a near tie"
            break
    assert r["sequence_lengths"].tolist() == o["sequence_lengths"].tolist()


@pytest.mark.one_decode_path
@pytest.mark.parametrize("int8_mode", [0, 1])
def test_sequential_residual_layers_follow_hf_and_oracle(gh, tiny, int8_mode):
    """use_gptj_residual = 0: h = attn + bias + x ; x' = ffn(LN2(h)) + bias + h (GptNeoXDecoder.cc:313-331,362-367); the
    engine runs these layers on its general path.  Pinned by HF's use_parallel_residual=False model."""
    from tests.test_oracle_golden import _sequential_weights
    cfg, w, _, _, z = tiny
    w2, s = _sequential_weights(cfg, w)
    layers, glob = weight_list_to_layers(cfg, w2)
    if int8_mode:
        layers = quantize_layers(layers)
    op = gh.make_op(cfg, w2, int8_mode=int8_mode, use_gptj_residual=False)
    B = 2
    ids = np.stack([z["prompt"], z["prompt"][::-1]]).astype(np.int32)
    r = gh.run_op(op, ids, [16, 16], 8, cfg["vocab_size"], top_k=1)
    assert op.stats()["decode_path"] == 2
    o = orc.Model(dict(cfg, fp16=1, int8_mode=int8_mode, use_gptj_residual=0), layers, glob).generate(
        ids, [16, 16], 8, return_logits=True)
    for b in range(B):
        for t in range(8):
            _logit_close(r["logits"][t, b], o["logits"][t, b])
            if r["output_ids"][b, 16 + t] != o["output_ids"][b, 16 + t]:
                top2 = np.sort(o["logits"][t, b])[-2:]
                assert top2[1] - top2[0] < 2 * LOGIT_FRAC * np.abs(o["logits"][t, b]).max(), "token flip without a near tie"
                break
    if not int8_mode:
        assert r["output_ids"][0, 16:].tolist() == s["hf_tokens"].tolist()


def test_one_engine_serves_requests_of_changing_shape(gh, tiny):
    """The arena is re-planned per request (and may grow), graphs are re-captured, hand-off slabs / split-K tickets are reset:
    a request must not depend on what ran before it."""
    from tests.test_gpu_beam import _replay
    cfg, w, layers, glob, z = tiny
    op = gh.make_op(cfg, w)
    m = orc.Model(dict(cfg, fp16=1), layers, glob)
    V = cfg["vocab_size"]
    rng = np.random.RandomState(3)
    first = None
    for B, S, out, K in [(1, 16, 8, 1), (5, 3, 4, 1), (2, 1, 6, 3), (1, 16, 8, 1), (16, 9, 5, 1), (3, 40, 3, 2), (33, 2, 3, 1),
                         (1, 16, 8, 1)]:
        if (B, S) == (1, 16):
            ids, lens = z["prompt"][None, :].astype(np.int32), np.array([16], np.int32)
        else:
            lens = rng.randint(1, S + 1, size=B).astype(np.int32)
            lens[0] = S
            ids = np.full((B, S), cfg["end_id"], np.int32)
            for b in range(B):
                ids[b, :lens[b]] = rng.randint(3, V, size=lens[b])
        if K > 1:
            r = gh.run_op_beam(op, ids, lens, out, V, K, return_logits=True)
            p_ids, _, _, _ = _replay(cfg, ids, lens, out, K, r["logits"], orc.BeamParams(B))
            assert r["output_ids"].tolist() == p_ids.tolist(), (B, S, out, K)
            continue
        r = gh.run_op(op, ids, lens, out, V, top_k=1)
        o = m.generate(ids, lens, out, return_logits=True)
        for b in range(B):
            for t in range(out):
                _logit_close(r["logits"][t, b], o["logits"][t, b])
                if o["output_ids"][b, lens[b] + t] == cfg["end_id"] or \
                        r["output_ids"][b, lens[b] + t] != o["output_ids"][b, lens[b] + t]:
                    break
        if (B, S) == (1, 16):
            first = r["output_ids"].copy() if first is None else first
            assert np.array_equal(first, r["output_ids"])
            assert r["output_ids"][0, 16:].tolist() == z["hf_tokens"].tolist()


def test_persistent_kernel_long_key_ranges(gh, tiny, monkeypatch, decode_path):
    """KV splits of more than 8 wave-loads of keys per lane (here 704 keys at size_per_head 64 with 24 workgroups, 6 splits)
    select the 16-deep instantiation of the persistent kernel's attention (rows held in the weight stream's register
    batches); logits follow the oracle.  (The 13B shape takes that form on the full grid: tests/test_gpu_fullsize.py.)"""
    if decode_path != "persistent":
        pytest.skip("persistent path only")
    monkeypatch.setenv("FTCF_PERSIST_NB", "24")
    cfg, w, layers, glob, z = tiny
    op = gh.make_op(cfg, w)
    S, out = 4200, 5
    ids = np.random.RandomState(6).randint(3, cfg["vocab_size"], size=(1, S)).astype(np.int32)
    r = gh.run_op(op, ids, [S], out, cfg["vocab_size"], top_k=1)
    assert op.stats()["decode_path"] == 1
    o = orc.Model(dict(cfg, fp16=1), layers, glob).generate(ids, [S], out, return_logits=True)
    for t in range(out):
        _logit_close(r["logits"][t, 0], o["logits"][t, 0])
        if r["output_ids"][0, S + t] != o["output_ids"][0, S + t]:
            top2 = np.sort(o["logits"][t, 0])[-2:]
            assert top2[1] - top2[0] < 2 * LOGIT_FRAC * np.abs(o["logits"][t, 0]).max(), "token flip without a near tie"
            break


@pytest.mark.one_decode_path
@pytest.mark.parametrize("seed", range(4))
def test_sampling_kernels_reproduce_the_oracle_given_the_same_logits(gh, tiny, seed):
    """The GPU's own per-step logits pushed through the oracle's dynamic decode (same counter-based uniforms, same (value
    desc, index asc) ordering): top-k / top-p / temperature / repetition-penalty sampling must pick the same tokens -- no
    model noise in this comparison, only exp/sum rounding at a cumulative boundary could differ."""
    cfg, w, layers, glob, z = tiny
    rng = np.random.RandomState(50 + seed)
    B, S, out = 4, 16, 10
    V = cfg["vocab_size"]
    ids = np.stack([np.roll(z["prompt"], i) for i in range(B)]).astype(np.int32)
    kw = dict(top_k=[int(x) for x in rng.choice([0, 1, 3, 8, 50], size=B)],
              top_p=[float(x) for x in rng.choice([0.0, 0.3, 0.8, 0.95], size=B)],
              temperature=[float(x) for x in rng.choice([0.6, 1.0, 1.4], size=B)],
              repetition_penalty=[float(x) for x in rng.choice([1.0, 1.15, 1.5], size=B)],
              random_seed=[int(x) for x in rng.randint(0, 1 << 30, size=B)])
    op = gh.make_op(cfg, w)
    r = gh.run_op(op, ids, [S] * B, out, V, **kw)
    sp = orc.Sampling(B, **kw)
    total = S + out
    step_ids = np.zeros((total, B), np.int32)
    step_ids[:S] = ids.T
    fin = np.zeros(B, np.uint8)
    seq = np.full(B, S - 1, np.int32)
    cum = np.zeros(B, np.float32)
    draws = np.zeros(B, np.uint64)
    lens = np.full(B, S, np.int32)
    mismatches = 0
    for t in range(out):
        lg = np.ascontiguousarray(r["logits"][t], dtype=np.float32).copy()
        orc.dynamic_decode(lg, S + t, S, lens, sp, cfg["end_id"], step_ids, fin, seq, cum, draws)
        got = r["output_ids"][:, S + t]
        bad = step_ids[S + t] != got
        if bad.any():  # keep the replay on the GPU's trajectory (penalties look at the history)
            mismatches += int(bad.sum())
            step_ids[S + t] = got
            fin[:] = np.where(bad, (got == cfg["end_id"]).astype(np.uint8), fin)
        if fin.all():
            break
    assert mismatches <= 1, (mismatches, kw)
    if mismatches == 0:
        # cum_log_probs of sampled rows (the reference's addBiasSoftMax + log of the drawn probability).  Top-k rows take the
        # row's max / sum of exponentials from per-slice statistics recombined in k_sample instead of one full-row soft-max:
        # the summation order differs from the oracle's, the values agree to fp32 rounding -- 1e-4 absolute on sums of <= 10 logs
        np.testing.assert_allclose(r["cum_log_probs"], cum, rtol=1e-4, atol=1e-4)


def test_begin_step_finish_equals_forward(gh, tiny):
    """ftcf_gptneox_forward == begin + step(...) + finish (include/ftcf.h): the token loop may be driven in pieces."""
    import ctypes as C
    import torch
    from fastertransformer4codefuse_amd import capi
    cfg, w, layers, glob, z = tiny
    op = gh.make_op(cfg, w)
    B, S, out = 2, 16, 8
    ids_np = np.stack([z["prompt"], z["prompt"][::-1]]).astype(np.int32)
    ref = gh.run_op(op, ids_np, [S] * B, out, cfg["vocab_size"], top_k=1, return_logits=False)
    ids = torch.from_numpy(ids_np).cuda()
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
    out_ids = torch.zeros((B, 1, S + out), dtype=torch.int32, device="cuda")
    seq = torch.zeros((B, 1), dtype=torch.int32, device="cuda")
    top_k = np.array([1], np.int32)
    fa = capi.ForwardArgs()
    fa.input_ids, fa.input_lengths = ids.data_ptr(), lens.data_ptr()
    fa.batch_size, fa.max_input_len, fa.output_len, fa.beam_width = B, S, out, 1
    fa.top_k, fa.n_top_k = top_k.ctypes.data, 1
    fa.output_ids, fa.sequence_lengths = out_ids.data_ptr(), seq.data_ptr()
    L = capi.lib()
    done = C.c_int(0)
    assert L.ftcf_gptneox_step(op._h, 1, C.byref(done)) != 0  # no request in flight
    capi.check(L.ftcf_gptneox_begin(op._h, C.byref(fa)))
    total_done = 0
    for n in (3, 2, 100):
        capi.check(L.ftcf_gptneox_step(op._h, n, C.byref(done)))
        assert done.value <= n
        total_done += done.value
    assert total_done == out
    capi.check(L.ftcf_gptneox_finish(op._h))
    torch.cuda.synchronize()
    assert out_ids[:, 0].cpu().numpy().tolist() == ref["output_ids"].tolist()
    assert seq[:, 0].cpu().numpy().tolist() == ref["sequence_lengths"].tolist()


@pytest.mark.one_decode_path
def test_invalid_requests_raise_and_leave_the_engine_usable(gh, tiny):
    """Argument errors come back as exceptions with a message (the reference TORCH_CHECKs / exits); the engine keeps working."""
    import torch
    from fastertransformer4codefuse_amd.capi import FtcfError
    cfg, w, layers, glob, z = tiny
    op = gh.make_op(cfg, w)
    ids = torch.from_numpy(z["prompt"][None, :].astype(np.int32)).cuda()
    lens = torch.tensor([16], dtype=torch.int32, device="cuda")
    with pytest.raises((RuntimeError, FtcfError)):
        op.forward(ids, lens, 0)  # output_len must be >= 1
    with pytest.raises((RuntimeError, FtcfError)):
        op.forward(ids, lens, 4, 1, torch.tensor([1, 2, 3], dtype=torch.int32))  # top_k of size 3 for batch 1
    with pytest.raises((RuntimeError, FtcfError)):
        op.forward(ids.cpu(), lens, 4)  # host tensor
    with pytest.raises((RuntimeError, FtcfError)):
        op.forward(ids.to(torch.int64), lens, 4)  # wrong dtype
    r = gh.run_op(op, z["prompt"][None, :], [16], 8, cfg["vocab_size"], top_k=1, return_logits=False)
    assert r["output_ids"][0, 16:].tolist() == z["hf_tokens"].tolist()


@pytest.mark.one_decode_path
@pytest.mark.parametrize("int8_mode", [0, 1])
def test_mid_model_long_ragged_prefill(gh, int8_mode):
    """Prefill kernels on shapes that cross their tile sizes: 257 / 130-token prompts (64-query and 64-key tiles of the MFMA
    attention, 128-row tiles of the GEMM), size_per_head 128, ragged batch."""
    cfg = MID
    w = random_model(cfg, seed=77 + int8_mode, std=0.04)
    layers, glob = weight_list_to_layers(cfg, w)
    if int8_mode:
        layers = quantize_layers(layers)
    rng = np.random.RandomState(9)
    S, out = 257, 4
    lens = np.array([257, 130], np.int32)
    ids = np.full((2, S), cfg["end_id"], dtype=np.int32)
    for b in range(2):
        ids[b, :lens[b]] = rng.randint(3, cfg["vocab_size"], size=lens[b])
    op = gh.make_op(cfg, w, int8_mode=int8_mode)
    r = gh.run_op(op, ids, lens, out, cfg["vocab_size"], top_k=1)
    o = orc.Model(dict(cfg, fp16=1, int8_mode=int8_mode), layers, glob).generate(ids, lens, out, return_logits=True)
    for b in range(2):
        for t in range(out):
            _logit_close(r["logits"][t, b], o["logits"][t, b])
            if r["output_ids"][b, lens[b] + t] != o["output_ids"][b, lens[b] + t]:
                top2 = np.sort(o["logits"][t, b])[-2:]
                assert top2[1] - top2[0] < 2 * LOGIT_FRAC * np.abs(o["logits"][t, b]).max(), "token flip without a near tie"
                break


def test_request_is_replayed_off_the_persistent_path_when_its_kernel_gives_up(gh, tiny, monkeypatch, decode_path):
    """The persistent kernel reports a hand-off it gave up on through a sticky error word (bounded spins, no hang);
    forward() then replays the request on the per-stage path and the engine stays there (FTCF_PERSIST_FAIL_ONCE is the
    test hook that raises the error word once)."""
    if decode_path != "persistent":
        pytest.skip("persistent path only")
    cfg, w, layers, glob, z = tiny
    monkeypatch.setenv("FTCF_PERSIST_FAIL_ONCE", "1")
    op = gh.make_op(cfg, w)
    r = gh.run_op(op, z["prompt"][None, :], [16], 8, cfg["vocab_size"], top_k=1)
    assert op.stats()["decode_path"] == 0  # the replay ran the per-stage launches
    assert r["output_ids"][0, 16:].tolist() == z["hf_tokens"].tolist()
    r2 = gh.run_op(op, z["prompt"][None, :], [16], 8, cfg["vocab_size"], top_k=1)
    assert op.stats()["decode_path"] == 0 and r2["output_ids"].tolist() == r["output_ids"].tolist()


def test_begin_without_finish_then_a_new_request(gh, tiny):
    """A request left open (begin + step, no finish) must not leak its captured graph into the next request."""
    import ctypes as C
    import torch
    from fastertransformer4codefuse_amd import capi
    cfg, w, layers, glob, z = tiny
    op = gh.make_op(cfg, w)
    ref = gh.run_op(op, z["prompt"][None, :], [16], 8, cfg["vocab_size"], top_k=1)
    ids = torch.from_numpy(np.ascontiguousarray(z["prompt"][None, :], dtype=np.int32)).cuda()
    lens = torch.tensor([16], dtype=torch.int32).cuda()
    out_ids = torch.empty((1, 1, 40), dtype=torch.int32, device="cuda")
    seq = torch.empty((1, 1), dtype=torch.int32, device="cuda")
    top_k = np.array([1], np.int32)
    fa = capi.ForwardArgs()
    fa.input_ids, fa.input_lengths = ids.data_ptr(), lens.data_ptr()
    fa.batch_size, fa.max_input_len, fa.output_len, fa.beam_width = 1, 16, 24, 1  # a different total length
    fa.top_k, fa.n_top_k = top_k.ctypes.data, 1
    fa.output_ids, fa.sequence_lengths = out_ids.data_ptr(), seq.data_ptr()
    capi.check(capi.lib().ftcf_gptneox_begin(op._h, C.byref(fa)))
    capi.check(capi.lib().ftcf_gptneox_step(op._h, 5, None))  # ... and never finished
    again = gh.run_op(op, z["prompt"][None, :], [16], 8, cfg["vocab_size"], top_k=1)
    assert again["output_ids"].tolist() == ref["output_ids"].tolist()
    np.testing.assert_array_equal(again["logits"], ref["logits"])


def test_fp16_kernels_can_be_retiled_in_place(gh, tiny, monkeypatch):
    """FTCF_FP16_RETILE_IN_PLACE=1: the engine overwrites the caller's row-major fp16 kernels with its tile image instead of
    keeping a second copy (52 GB instead of 26 GB at 13B); same tokens and logits as the default."""
    cfg, w, layers, glob, z = tiny
    r0 = gh.run_op(gh.make_op(cfg, w), z["prompt"][None, :], [16], 8, cfg["vocab_size"], top_k=1)
    monkeypatch.setenv("FTCF_FP16_RETILE_IN_PLACE", "1")
    op = gh.make_op(cfg, w)
    r1 = gh.run_op(op, z["prompt"][None, :], [16], 8, cfg["vocab_size"], top_k=1)
    assert r1["output_ids"].tolist() == r0["output_ids"].tolist()
    np.testing.assert_array_equal(r1["logits"], r0["logits"])
    L, H = cfg["num_layer"], cfg["head_num"] * cfg["size_per_head"]
    # the caller's QKV kernel of layer 0 no longer holds the row-major matrix
    assert not np.array_equal(op.weights[2 * L].cpu().numpy().astype(np.float32).reshape(H, 3 * H),
                              np.asarray(w[2 * L], np.float32).reshape(H, 3 * H).astype(np.float16).astype(np.float32))


@pytest.mark.parametrize("B", [1, 2])
def test_multi_token_graphs_equal_single_token_graphs(gh, tiny, monkeypatch, decode_path, B):
    """FTCF_GRAPH_TOKENS tokens per captured graph (default 8; persistent path): the same tokens, lengths and LOOP COUNT as one
    token per graph -- also when the rows finish on end_id in the middle of a graph (the launches behind the last token return at
    once on the device's flag and the host's counters are set back to the device's: GptNeoX.cc:776-1048 leaves its loop at that
    token), and when the token loop is driven in pieces through begin / step / finish."""
    import ctypes as C
    import torch
    from fastertransformer4codefuse_amd import capi
    if decode_path != "persistent":
        pytest.skip("persistent-path-only")
    cfg, w, layers, glob, z = tiny
    S, out = 16, 30
    ids_np = np.stack([z["prompt"], z["prompt"][::-1]]).astype(np.int32)[:B]
    monkeypatch.setenv("FTCF_GRAPH_TOKENS", "1")
    free = gh.run_op(gh.make_op(cfg, w), ids_np, [S] * B, out, cfg["vocab_size"], top_k=1, return_logits=False)
    # an end_id that row 0 emits as its 6th new token: with 4 tokens per graph the request ends in the middle of a graph
    cfg2 = dict(cfg, end_id=int(free["output_ids"][0, S + 5]))
    res = {}
    for n in (1, 4, 8):
        monkeypatch.setenv("FTCF_GRAPH_TOKENS", str(n))
        op = gh.make_op(cfg2, w)
        r = gh.run_op(op, ids_np, [S] * B, out, cfg["vocab_size"], top_k=1, return_logits=False)
        res[n] = (r["output_ids"].tolist(), r["sequence_lengths"].tolist(), r["cum_log_probs"].tolist(), op.stats()["decode_steps"])
        rf = gh.run_op(gh.make_op(cfg, w), ids_np, [S] * B, out, cfg["vocab_size"], top_k=1, return_logits=False)
        assert rf["output_ids"].tolist() == free["output_ids"].tolist()  # (no early end: whole graphs + single-token tail)
    assert res[4] == res[1] and res[8] == res[1], (res[1][3], res[4][3], res[8][3])
    if B == 1:
        assert res[1][3] == 6  # the loop count of the reference: it leaves its loop at the token that finished the last row
    # the loop in pieces: 3 + 9 + the rest, four tokens per graph
    monkeypatch.setenv("FTCF_GRAPH_TOKENS", "4")
    op = gh.make_op(cfg2, w)
    ids = torch.from_numpy(ids_np).cuda()
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
    out_ids = torch.zeros((B, 1, S + out), dtype=torch.int32, device="cuda")
    seq = torch.zeros((B, 1), dtype=torch.int32, device="cuda")
    top_k = np.array([1], np.int32)
    fa = capi.ForwardArgs()
    fa.input_ids, fa.input_lengths = ids.data_ptr(), lens.data_ptr()
    fa.batch_size, fa.max_input_len, fa.output_len, fa.beam_width = B, S, out, 1
    fa.top_k, fa.n_top_k = top_k.ctypes.data, 1
    fa.output_ids, fa.sequence_lengths = out_ids.data_ptr(), seq.data_ptr()
    L = capi.lib()
    done, total_done = C.c_int(0), 0
    capi.check(L.ftcf_gptneox_begin(op._h, C.byref(fa)))
    for n in (3, 9, 100):
        capi.check(L.ftcf_gptneox_step(op._h, n, C.byref(done)))
        assert 0 <= done.value <= n
        total_done += done.value
    capi.check(L.ftcf_gptneox_finish(op._h))
    torch.cuda.synchronize()
    assert out_ids[:, 0].cpu().numpy().tolist() == res[1][0] and seq[:, 0].cpu().numpy().tolist() == res[1][1]
    assert total_done == res[1][3]


def _forward_capi(op, ids_np, S, out, V, min_length=None, stop_words=None):
    """A request through the C ABI's argument block (min_length is not reachable through GptNeoXOp.forward)."""
    import ctypes as C
    import torch
    from fastertransformer4codefuse_amd import capi
    B = ids_np.shape[0]
    ids = torch.from_numpy(np.ascontiguousarray(ids_np, dtype=np.int32)).cuda()
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
    out_ids = torch.zeros((B, 1, S + out), dtype=torch.int32, device="cuda")
    seq = torch.zeros((B, 1), dtype=torch.int32, device="cuda")
    cum = torch.zeros((B, 1), dtype=torch.float32, device="cuda")
    top_k = np.array([1], np.int32)
    fa = capi.ForwardArgs()
    fa.input_ids, fa.input_lengths = ids.data_ptr(), lens.data_ptr()
    fa.batch_size, fa.max_input_len, fa.output_len, fa.beam_width = B, S, out, 1
    fa.top_k, fa.n_top_k = top_k.ctypes.data, 1
    if min_length is not None:
        ml = np.ascontiguousarray(min_length, dtype=np.int32)
        fa.min_length, fa.n_min_length = ml.ctypes.data, ml.size
    if stop_words is not None:
        sw = torch.from_numpy(np.ascontiguousarray(stop_words, dtype=np.int32)).cuda()
        fa.stop_words_list, fa.stop_words_len = sw.data_ptr(), stop_words.shape[2]
    fa.return_cum_log_probs = 1
    fa.output_ids, fa.sequence_lengths, fa.cum_log_probs = out_ids.data_ptr(), seq.data_ptr(), cum.data_ptr()
    capi.check(capi.lib().ftcf_gptneox_forward(op._h, C.byref(fa)))
    torch.cuda.synchronize()
    return out_ids[:, 0].cpu().numpy(), seq[:, 0].cpu().numpy(), cum[:, 0].cpu().numpy(), op.stats()["decode_steps"]


GREEDY_FORMS = {"lm-head launch": ("1", "1"), "one launch": ("0", "1"), "four launches": ("0", "0")}


@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_the_three_forms_of_an_all_greedy_step_agree_and_follow_the_oracle(gh, tiny, monkeypatch, B):
    """An all-greedy step runs (a) inside the LM head launch (k_lm_head_greedy: <= 2 rows on one GPU; three and four rows take form (b)), (b) as one launch behind
    k_lm_head (k_greedy_decode), (c) as the general four launches.  Same tokens, lengths and loop count from all three, scores to
    1e-4 -- on a request whose rows end on end_id at different steps, with min_length holding the end token back (the mask of
    sampling_penalty_kernels.cu:485-520, which the bench's request uses and GptNeoXOp.forward cannot reach) and with stop
    words -- and all of it what the oracle generates."""
    from oracle import oracle as orc
    cfg, w, layers, glob, z = tiny
    V, S, out = cfg["vocab_size"], 16, 14
    # rows whose free-running greedy tokens the engine and the oracle agree on (the tiny model's logits are flat: a near tie may
    # fall either way in fp16, and everything behind a flipped token differs): the golden prompt first, then candidates
    rng = np.random.RandomState(12)
    pool = [z["prompt"], z["prompt"][::-1], np.roll(z["prompt"], 5), np.roll(z["prompt"][::-1], 3)]
    pool += [rng.randint(3, V, size=S) for _ in range(8)]
    pool = np.stack([np.asarray(r, np.int32)[:S] for r in pool])
    n = len(pool)
    eng_free = gh.run_op(gh.make_op(cfg, w), pool, [S] * n, out, V, top_k=1, return_logits=False)["output_ids"]
    orc_free = orc.Model(dict(cfg, fp16=1), layers, glob).generate(pool, [S] * n, out, orc.Sampling(n, top_k=1))["output_ids"]
    keep = [i for i in range(n) if np.array_equal(eng_free[i], orc_free[i])]
    assert keep and keep[0] == 0 and len(keep) >= B, keep
    ids_np = pool[keep[:B]]
    free = eng_free[keep[:B]]
    cfg2 = dict(cfg, end_id=int(free[0, S + 3]))  # row 0 emits it as its 4th new token
    model = orc.Model(dict(cfg2, fp16=1), layers, glob)
    stop = np.full((B, 2, 4), -1, np.int32)
    stop[:, 0, :] = 0
    for b in range(B):  # every row stops on ITS 6th and 7th free-running tokens
        stop[b, 0, :2] = free[b, S + 5:S + 7]
        stop[b, 1, 0] = 2
    cases = {"end_id": {}, "min_length": dict(min_length=[9] * B), "stop_words": dict(stop_words=stop, min_length=[20] * B)}
    for name, kw in cases.items():
        ref = model.generate(ids_np, [S] * B, out, orc.Sampling(B, top_k=1, **kw))
        got = {}
        for form, (lm, fused) in GREEDY_FORMS.items():
            monkeypatch.setenv("FTCF_LM_GREEDY", lm)
            monkeypatch.setenv("FTCF_GREEDY_FUSED", fused)
            got[form] = _forward_capi(gh.make_op(cfg2, w), ids_np, S, out, V, **kw)
        base = got["four launches"]
        for form, g in got.items():
            assert np.array_equal(g[0], base[0]) and np.array_equal(g[1], base[1]) and g[3] == base[3], (name, form, g, base)
            np.testing.assert_allclose(g[2], base[2], rtol=1e-4, atol=1e-4, err_msg=f"{name} {form}")
        assert np.array_equal(base[0], ref["output_ids"]), (name, base[0], ref["output_ids"])
        assert np.array_equal(base[1], ref["sequence_lengths"]), (name, base[1], ref["sequence_lengths"])
        # (scores end to end: sums of up to 14 log-probabilities of fp16 logits computed in two summation orders)
        np.testing.assert_allclose(base[2], ref["cum_log_probs"], rtol=2e-2, atol=5e-2, err_msg=name)
        assert base[3] == ref["steps"], (name, base[3], ref["steps"])
        if name == "min_length":
            assert (base[1] - S >= 9).all()  # nobody ended before its ninth new token ...
            assert not np.array_equal(base[0], got_end[0])  # ... where the unmasked request did
        if name == "end_id":
            got_end = base
