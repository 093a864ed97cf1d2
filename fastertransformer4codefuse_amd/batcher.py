"""Continuous batching over a paged K/V cache (include/ftcf.h `ftcf_batcher_*`).

    op = GptNeoXOp(...)                       # fp16 / int8 engine, tensor_para_size 1
    cb = ContinuousBatcher(op, max_batch=8, page_tokens=64, num_pages=512, max_seq_len=2048)
    rid = cb.submit(prompt_ids, max_new_tokens=128)          # greedy; top_k / top_p / temperature / seed /
                                                             # repetition_penalty / stop_words optional
    cb.submit(prompt_ids, 128, logit_bias={id: -inf}, bad_words=[[a, b]], presence_penalty=.5, frequency_penalty=.2,
              min_new_tokens=8)                              # per-request logit processors
    cb.set_token_mask(rid, allowed_ids)                      # the next tokens come from this set (grammar-constrained decoding)
    rids = cb.submit_n(prompt_ids, 128, n=8, top_k=40, seed=1) # 8 samples of one prompt from ONE prompt phase (seed + i each);
                                                             # the prompt's full pages are shared (fork_stats())
    bid = cb.submit_beam(prompt_ids, 128, beam_width=4)      # beam search: one event (bid, -1, True), then cb.beam_result(bid)
    ContinuousBatcher(op, ..., prefix_cache=True)             # reuse the K/V pages of shared prompt prefixes (prefix_stats())
    ContinuousBatcher(op, ..., overcommit=True, swap_pages=0) # pages on demand, the latest arrival swapped to host memory when
                                                             # the pool runs dry (preempt_stats()); streams stay exact
    while cb.busy():
        for request_id, token, finished in cb.step():
            ...

The engine `op` must not run a request of its own while a batcher call is in progress."""
import ctypes as C

import numpy as np

from . import capi


def _word_list(words):
    """token-id lists -> the [2, n] word list of to_word_list_format (codefuse_example.py:26-53)"""
    flat = [int(t) for w in words for t in w]
    arr = np.zeros((2, len(flat)), dtype=np.int32)
    arr[0] = flat
    arr[1] = -1
    arr[1, :len(words)] = np.cumsum([len(w) for w in words])
    return np.ascontiguousarray(arr)


def pack_logit_options(logit_bias=None, bad_words=None, presence_penalty=0.0, frequency_penalty=0.0, min_new_tokens=0):
    """The logit-processor keywords of submit() as (ftcf_logit_options, the arrays it points to), or (None, ()) when none is
    set.  What can be checked without the vocabulary size is checked here (ValueError); ids >= V are the library's to refuse."""
    pairs = list(logit_bias.items()) if isinstance(logit_bias, dict) else [tuple(p) for p in (logit_bias or ())]
    ids = [int(i) for i, _ in pairs]
    vals = [float(v) for _, v in pairs]
    words = [list(w) for w in (bad_words or ())]
    presence_penalty, frequency_penalty = float(presence_penalty), float(frequency_penalty)
    if len(ids) > 1024:
        raise ValueError("logit_bias takes at most 1024 pairs")
    if len(set(ids)) != len(ids):
        raise ValueError("logit_bias: duplicate token id")
    if any(i < 0 for i in ids):
        raise ValueError("logit_bias: token id out of range")
    if any(np.isnan(v) or v == np.inf for v in vals):
        raise ValueError("logit_bias: a value is NaN or +inf")
    if not (np.isfinite(presence_penalty) and np.isfinite(frequency_penalty)):
        raise ValueError("presence_penalty and frequency_penalty must be finite")
    if int(min_new_tokens) != min_new_tokens or min_new_tokens < 0:
        raise ValueError("min_new_tokens must be a non-negative integer")
    if any(len(w) == 0 for w in words) or any(t < 0 for w in words for t in w):
        raise ValueError("bad_words: an empty word or a negative token id")
    if sum(len(w) for w in words) > 256:
        raise ValueError("bad_words holds at most 256 tokens")
    if not (ids or words or presence_penalty != 0.0 or frequency_penalty != 0.0 or min_new_tokens):
        return None, ()
    o = capi.LogitOptions()
    o.struct_size = C.sizeof(capi.LogitOptions)
    o.presence_penalty, o.frequency_penalty, o.min_new_tokens = presence_penalty, frequency_penalty, int(min_new_tokens)
    keep = []
    if ids:
        a, v = np.asarray(ids, dtype=np.int32), np.asarray(vals, dtype=np.float32)
        o.bias_ids, o.bias_values, o.n_bias = a.ctypes.data_as(C.POINTER(C.c_int)), v.ctypes.data_as(C.POINTER(C.c_float)), len(ids)
        keep += [a, v]
    if words:
        w = _word_list(words)
        o.bad_words, o.bad_words_len = w.ctypes.data_as(C.POINTER(C.c_int)), int(w.shape[1])
        keep.append(w)
    return o, tuple(keep)


class ContinuousBatcher:
    def __init__(self, op, max_batch, page_tokens, num_pages, max_seq_len, prefix_cache=False, overcommit=False, swap_pages=0):
        """prefix_cache=True: full prompt blocks of page_tokens tokens stay cached in the pool and later prompts that start with
        them reuse their K/V (ftcf_batcher_create_ex); refused for tensor_para_size > 1 and fp32 engines.
        overcommit=True (ftcf_batcher_create_opts): requests take pages as their sequences grow instead of reserving
        prompt + max_new_tokens at admission; when the pool runs dry the latest arrival is swapped out to swap_pages pinned host
        pages (0: num_pages) and resumes later, token for token as if it had never left (preempt_stats()); refused for
        tensor_para_size > 1."""
        self._op = op  # keeps the engine (and its weights) alive
        self.max_batch = int(max_batch)
        self._h = C.c_void_p()
        if overcommit:
            o = capi.BatcherOptions()
            o.struct_size = C.sizeof(capi.BatcherOptions)
            o.max_batch, o.page_tokens, o.num_pages, o.max_seq_len = int(max_batch), int(page_tokens), int(num_pages), int(max_seq_len)
            o.prefix_cache, o.overcommit, o.swap_pages, o.swap_stage_bytes = int(bool(prefix_cache)), 1, int(swap_pages), 0
            capi.check(capi.lib().ftcf_batcher_create_opts(op._h, C.byref(o), C.byref(self._h)))
        elif prefix_cache:
            capi.check(capi.lib().ftcf_batcher_create_ex(op._h, int(max_batch), int(page_tokens), int(num_pages), int(max_seq_len), 1,
                                                         C.byref(self._h)))
        else:
            capi.check(capi.lib().ftcf_batcher_create(op._h, int(max_batch), int(page_tokens), int(num_pages), int(max_seq_len),
                                                      C.byref(self._h)))
        n = 2 * self.max_batch  # (a chunked admission can produce more events per iteration: the rest comes with the next call)
        self._ids = (C.c_long * n)()
        self._tok = (C.c_int * n)()
        self._fin = (C.c_int * n)()
        self._lp = (C.c_float * n)()
        self._cb = None
        self._beam_log_probs = {}  # request id -> max_new_tokens of the beam requests submitted with token_log_probs

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                capi.lib().ftcf_batcher_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def submit(self, prompt_ids, max_new_tokens, top_k=0, top_p=0.0, temperature=1.0, seed=0, repetition_penalty=1.0,
               stop_words=None, *, logit_bias=None, bad_words=None, presence_penalty=0.0, frequency_penalty=0.0, min_new_tokens=0):
        """stop_words: a list of token-id lists (each one a stop sequence), or None.  The request ends after a stop
        sequence has been emitted (stop_criteria_kernels.cu:24-83), like GptNeoXOp.forward with stop_words_list.

        Logit processors (ftcf_batcher_submit_opts; applied to every token of the request, the first included, in this order,
        before the sampling parameters): presence_penalty / frequency_penalty over the GENERATED tokens (additive, OpenAI
        semantics), logit_bias ({token id: value} or (id, value) pairs, at most 1024; -inf bans a token), min_new_tokens (the end
        token is held back that long), bad_words (token-id lists as stop_words: a one-token word is banned, a longer one may not
        be completed).  set_token_mask() adds the per-step allowed-token mask."""
        opts, keep = pack_logit_options(logit_bias, bad_words, presence_penalty, frequency_penalty, min_new_tokens)
        ids = np.ascontiguousarray(prompt_ids, dtype=np.int32).reshape(-1)
        rid = C.c_long(0)
        sw = _word_list(stop_words) if stop_words else None
        sw_len = int(sw.shape[1]) if sw is not None else 0
        request = (self._h, capi.vp(ids), int(ids.size), int(max_new_tokens), int(top_k), top_p, temperature, repetition_penalty,
                   int(seed), capi.vp(sw), sw_len)
        if opts is not None:
            capi.check(capi.lib().ftcf_batcher_submit_opts(*request, C.byref(opts), C.byref(rid)))
            del keep  # (the call copies the arrays)
            return int(rid.value)
        capi.check(capi.lib().ftcf_batcher_submit_ex(*request, C.byref(rid)))
        return int(rid.value)

    def submit_n(self, prompt_ids, max_new_tokens, n, top_k=0, top_p=0.0, temperature=1.0, seed=0, repetition_penalty=1.0,
                 stop_words=None, *, logit_bias=None, bad_words=None, presence_penalty=0.0, frequency_penalty=0.0, min_new_tokens=0):
        """n samples of one prompt (ftcf_batcher_submit_n): ONE fork request, the list of its n request ids.  Sibling i is the
        request submit() with seed + i would be and produces exactly its tokens; the prompt runs through the model once and its
        full pages are shared (fork_stats()).  The other arguments are submit()'s.  From its first token on a sibling is an
        ordinary request (events, cancel, set_token_mask, ...); while the fork waits, cancel(id) drops that sibling and
        set_token_mask(id, ...) sets that sibling's own mask."""
        opts, keep = pack_logit_options(logit_bias, bad_words, presence_penalty, frequency_penalty, min_new_tokens)
        ids = np.ascontiguousarray(prompt_ids, dtype=np.int32).reshape(-1)
        n = int(n)
        rids = (C.c_long * max(n, 1))()
        sw = _word_list(stop_words) if stop_words else None
        capi.check(capi.lib().ftcf_batcher_submit_n(
            self._h, capi.vp(ids), int(ids.size), int(max_new_tokens), int(top_k), top_p, temperature, repetition_penalty,
            int(seed) % (1 << 64), capi.vp(sw), int(sw.shape[1]) if sw is not None else 0,
            C.byref(opts) if opts is not None else None, n, rids))
        del keep  # (the call copies the arrays)
        return [int(rids[i]) for i in range(n)]

    def fork_stats(self):
        """Counters of submit_n since creation: requests (fork admissions), siblings (the slots they opened), shared_pages (page
        allocations sharing saved) and prompt_tokens_computed (what their prompt phases ran: one prompt per fork, less its hit)."""
        r, s, p, t = C.c_long(0), C.c_long(0), C.c_long(0), C.c_long(0)
        capi.check(capi.lib().ftcf_batcher_fork_stats(self._h, C.byref(r), C.byref(s), C.byref(p), C.byref(t)))
        return {"requests": r.value, "siblings": s.value, "shared_pages": p.value, "prompt_tokens_computed": t.value}

    def set_token_mask(self, request_id, allowed):
        """The allowed-token mask of a waiting or running request (ftcf_batcher_set_token_mask): every token sampled for it from
        the next one on comes from `allowed` -- a bool array of length V or an iterable of token ids -- until the mask is
        replaced; None clears it.  May be called from inside the token callback (grammar-constrained decoding: advance the
        grammar on the event, hand the next step's mask back).  A request whose mask and options leave no token ends with end_id."""
        if allowed is None:
            capi.check(capi.lib().ftcf_batcher_set_token_mask(self._h, int(request_id), None, 0))
            return
        V = int(self._op.vocab_size_)
        a = np.asarray(allowed if isinstance(allowed, np.ndarray) else list(allowed))
        if a.dtype == np.bool_:
            if a.shape != (V,):
                raise ValueError("a bool mask has one entry per token of the vocabulary")
            bits = a
        else:
            a = a.astype(np.int64).reshape(-1)
            if a.size and (a.min() < 0 or a.max() >= V):
                raise ValueError("token mask: token id out of range")
            bits = np.zeros(V, dtype=np.bool_)
            bits[a] = True
        words = np.ascontiguousarray(np.packbits(np.pad(bits, (0, -V % 32)), bitorder="little").view(np.uint32))
        capi.check(capi.lib().ftcf_batcher_set_token_mask(self._h, int(request_id), capi.vp(words), int(words.size)))

    def submit_beam(self, prompt_ids, max_new_tokens, beam_width, beam_search_diversity_rate=0.0, len_penalty=0.0, temperature=1.0,
                    repetition_penalty=1.0, min_length=0, stop_words=None, token_log_probs=False):
        """A beam-search request (GptNeoXOp.forward with beam_width > 1).  step() reports one event for it, (request_id, -1, True),
        when it has finished; beam_result(request_id) then returns what forward returns for one prompt.  token_log_probs=True
        (ftcf_batcher_submit_beam_opts): beam_result also returns every hypothesis' per-token log-probabilities
        (GptNeoXOp.beam_log_probs)."""
        ids = np.ascontiguousarray(prompt_ids, dtype=np.int32).reshape(-1)
        rid = C.c_long(0)
        sw = _word_list(stop_words) if stop_words else None
        sw_len = int(sw.shape[1]) if sw is not None else 0
        if token_log_probs:
            o = capi.BeamOptions(C.sizeof(capi.BeamOptions), int(beam_width), beam_search_diversity_rate, len_penalty, temperature,
                                 repetition_penalty, int(min_length),
                                 sw.ctypes.data_as(C.POINTER(C.c_int)) if sw is not None else None, sw_len, 1)
            capi.check(capi.lib().ftcf_batcher_submit_beam_opts(self._h, capi.vp(ids), int(ids.size), int(max_new_tokens),
                                                                C.byref(o), C.byref(rid)))
            self._beam_log_probs[int(rid.value)] = int(max_new_tokens)
            return int(rid.value)
        capi.check(capi.lib().ftcf_batcher_submit_beam_ex(
            self._h, capi.vp(ids), int(ids.size), int(max_new_tokens), int(beam_width), beam_search_diversity_rate, len_penalty,
            temperature, repetition_penalty, int(min_length), capi.vp(sw), sw_len, C.byref(rid)))
        return int(rid.value)

    def beam_result(self, request_id):
        """(output_ids [beam_width, prompt_len + max_new_tokens], sequence_lengths [beam_width], cum_log_probs [beam_width]) of a
        finished beam request, once; None while it is running or when the id is unknown.  A request submitted with
        token_log_probs=True returns a fourth array, token_log_probs [beam_width, max_new_tokens] float32: entry i belongs to
        output_ids[:, prompt_len + i]; 0 behind a hypothesis' first end token and in the end_id padding."""
        k, t = C.c_int(0), C.c_int(0)
        capi.check(capi.lib().ftcf_batcher_beam_result(self._h, int(request_id), None, None, None, 0, C.byref(k), C.byref(t)))
        if k.value == 0:
            return None
        ids = np.zeros((k.value, t.value), dtype=np.int32)
        lens = np.zeros(k.value, dtype=np.int32)
        cum = np.zeros(k.value, dtype=np.float32)
        if int(request_id) in self._beam_log_probs:
            lp = np.zeros((k.value, self._beam_log_probs[int(request_id)]), dtype=np.float32)
            capi.check(capi.lib().ftcf_batcher_beam_result_ex(
                self._h, int(request_id), capi.vp(ids), capi.vp(lens), capi.vp(cum), capi.vp(lp), int(ids.size), C.byref(k), C.byref(t)))
            del self._beam_log_probs[int(request_id)]
            return ids, lens, cum, lp
        capi.check(capi.lib().ftcf_batcher_beam_result(
            self._h, int(request_id), capi.vp(ids), capi.vp(lens), capi.vp(cum), int(ids.size), C.byref(k), C.byref(t)))
        return ids, lens, cum

    def set_token_callback(self, fn):
        """fn(request_id, token, finished) is called from inside step() for every token the moment it is on the host (between
        the chunks of a long admission as well); None unsets.  The events are still returned by step()."""
        if fn is None:
            self._cb = None
            capi.check(capi.lib().ftcf_batcher_set_token_callback(self._h, C.cast(None, capi.BATCHER_TOKEN_CALLBACK), None))
            return
        self._cb = capi.BATCHER_TOKEN_CALLBACK(lambda _user, rid, tok, fin: fn(int(rid), int(tok), bool(fin)))
        capi.check(capi.lib().ftcf_batcher_set_token_callback(self._h, self._cb, None))

    def step(self, top_logprobs=None):
        """One scheduler iteration; returns [(request_id, token, finished), ...] in production order.

        top_logprobs = N in 1..20 (ftcf_batcher_step_top): the events are (request_id, token, finished, log_prob, top_ids,
        top_log_probs) -- log_prob as step_ex returns it, then the N most likely tokens of the distribution the token was
        drawn from, best first, and their log-probabilities (GptNeoXOp.forward's top_logprobs).  A beam request's event and
        events of admissions made by a call without it carry ids of -1 and NaN."""
        n = C.c_int(0)
        if top_logprobs:
            N, cap = int(top_logprobs), 2 * self.max_batch
            if not 1 <= N <= 20:
                raise ValueError("top_logprobs must be in 1..20")
            ids, lps = (C.c_int * (cap * N))(), (C.c_float * (cap * N))()
            capi.check(capi.lib().ftcf_batcher_step_top(self._h, self._ids, self._tok, self._fin, self._lp, N, ids, lps, cap, C.byref(n)))
            return [(int(self._ids[i]), int(self._tok[i]), bool(self._fin[i]), float(self._lp[i]), list(ids[i * N:(i + 1) * N]),
                     list(lps[i * N:(i + 1) * N])) for i in range(n.value)]
        capi.check(capi.lib().ftcf_batcher_step(self._h, self._ids, self._tok, self._fin, 2 * self.max_batch, C.byref(n)))
        return [(int(self._ids[i]), int(self._tok[i]), bool(self._fin[i])) for i in range(n.value)]

    def step_ex(self):
        """The same iteration with each token's log-probability: [(request_id, token, finished, log_prob), ...].  log_prob is
        the value the token adds to the request's cumulative log-probability (the engine's output_log_probs), NaN for a beam
        request's event."""
        n = C.c_int(0)
        capi.check(capi.lib().ftcf_batcher_step_ex(self._h, self._ids, self._tok, self._fin, self._lp, 2 * self.max_batch,
                                                   C.byref(n)))
        return [(int(self._ids[i]), int(self._tok[i]), bool(self._fin[i]), float(self._lp[i])) for i in range(n.value)]

    def status(self):
        w, r, f = C.c_int(0), C.c_int(0), C.c_int(0)
        capi.check(capi.lib().ftcf_batcher_status(self._h, C.byref(w), C.byref(r), C.byref(f)))
        return {"waiting": w.value, "running": r.value, "free_pages": f.value}

    def prefix_stats(self):
        """Counters of the prefix cache: enabled, cached_pages, evictable_pages, lookups, prompt_tokens, hit_tokens, computed_tokens,
        evictions (all 0 without the cache)."""
        en, cached, evictable = C.c_int(0), C.c_int(0), C.c_int(0)
        lk, pt, ht, ct, ev = C.c_long(0), C.c_long(0), C.c_long(0), C.c_long(0), C.c_long(0)
        capi.check(capi.lib().ftcf_batcher_prefix_stats(self._h, C.byref(en), C.byref(cached), C.byref(evictable), C.byref(lk),
                                                        C.byref(pt), C.byref(ht), C.byref(ct), C.byref(ev)))
        return {"enabled": en.value, "cached_pages": cached.value, "evictable_pages": evictable.value, "lookups": lk.value,
                "prompt_tokens": pt.value, "hit_tokens": ht.value, "computed_tokens": ct.value, "evictions": ev.value}

    def preempt_stats(self):
        """Counters of overcommit: enabled, swapped_requests (swapped out now), swap_pages_used, swap_pages_total, preemptions,
        resumes, pages_out, pages_in (all 0 without overcommit)."""
        en, sw, used, total = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        pre, res, po, pi = C.c_long(0), C.c_long(0), C.c_long(0), C.c_long(0)
        capi.check(capi.lib().ftcf_batcher_preempt_stats(self._h, C.byref(en), C.byref(sw), C.byref(used), C.byref(total),
                                                         C.byref(pre), C.byref(res), C.byref(po), C.byref(pi)))
        return {"enabled": en.value, "swapped_requests": sw.value, "swap_pages_used": used.value, "swap_pages_total": total.value,
                "preemptions": pre.value, "resumes": res.value, "pages_out": po.value, "pages_in": pi.value}

    def clear_prefix_cache(self):
        """Drops every cached page that no request is using (they return to the free list)."""
        capi.check(capi.lib().ftcf_batcher_clear_prefix_cache(self._h))

    def cancel(self, request_id):
        """Drops a waiting or running request; returns False when the id is unknown or already finished."""
        found = C.c_int(0)
        capi.check(capi.lib().ftcf_batcher_cancel(self._h, int(request_id), C.byref(found)))
        self._beam_log_probs.pop(int(request_id), None)  # (a cancelled beam request has no result to fetch)
        return bool(found.value)

    def busy(self):
        s = self.status()
        return s["waiting"] > 0 or s["running"] > 0

    def run_all(self, max_iterations=1 << 20):
        """Drains the queue; returns {request_id: [tokens]}."""
        out = {}
        it = 0
        while self.busy():
            for rid, tok, _ in self.step():
                if tok >= 0:  # (a beam request's only event carries -1: its hypotheses come from beam_result)
                    out.setdefault(rid, []).append(tok)
            it += 1
            if it > max_iterations:
                raise RuntimeError("the batcher did not drain")
        return out
