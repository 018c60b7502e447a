/*
 * minigpt4_amd.h -- ADDITIVE entry points of the MI355X build of libminigpt4.so.
 *
 * Nothing here changes the reference ABI (include/minigpt4.h).  These symbols exist for
 *   (1) measurement: device-resident decode loops timed with hipEvents, the per-launch-site table of the decode step, image-encode time;
 *   (2) token-level use of the language path (eval / logits / tokenize / sample) and the parity-mode switch;
 *   (3) batched / multi-GPU serving: the already-declared-but-unused MiniGPT4Images / MiniGPT4Embeddings carriers (reference minigpt4.h:80-90), several
 *       conversations per context, access to the weight arenas for a load-time RCCL broadcast.
 * Kernel-level test hooks, micro-benchmarks, hardware probes and host-only test helpers are NOT part of libminigpt4.so: they are declared in
 * minigpt4_amd_test.h and exported by libminigpt4_test.so (the same objects + csrc/test_hooks.cpp), which only tests/ and tools/ load.
 * Plain C types only (pointers + sizes); no torch / HIP types cross this boundary.
 */
#pragma once
#include "minigpt4.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- environment ------------------------------------------------------------------------------------------------ */
MINIGPT4_API int minigpt4_amd_device_count(void);                      /* 0 when no HIP device is usable */
MINIGPT4_API const char *minigpt4_amd_last_error(void);                /* thread-local text of the last failure */
MINIGPT4_API const char *minigpt4_amd_build_info(void);                /* "gfx950 ..." */

/* ---- language path, token level (parity tests; mirrors MiniGPT4::add_tokens / add_embedding / llama_get_logits) -- */
MINIGPT4_API int minigpt4_amd_n_vocab(struct MiniGPT4Context *ctx);
MINIGPT4_API int minigpt4_amd_n_embd(struct MiniGPT4Context *ctx);
MINIGPT4_API int minigpt4_amd_n_past(struct MiniGPT4Context *ctx);
MINIGPT4_API int minigpt4_amd_eval_tokens(struct MiniGPT4Context *ctx, const int32_t *tokens, int n);    /* 0 / 8 */
MINIGPT4_API int minigpt4_amd_eval_embd(struct MiniGPT4Context *ctx, const float *embd, int n_rows);      /* 0 / 10 */
MINIGPT4_API int minigpt4_amd_get_logits(struct MiniGPT4Context *ctx, float *out, size_t n);              /* last token's logits */
MINIGPT4_API int minigpt4_amd_tokenize(struct MiniGPT4Context *ctx, const char *text, int add_bos, int32_t *out, int cap); /* returns count */
MINIGPT4_API int minigpt4_amd_sample(struct MiniGPT4Context *ctx, int32_t *token_id, float temp, int32_t top_k, float top_p, float tfs_z, float typical_p,
                                     int mirostat, float mirostat_tau, float mirostat_eta);                 /* samples, does NOT eval */

/* Parity mode (also MINIGPT4_PARITY=1 in the environment at load): every fp32 accumulation of the language path in the CPU oracle's order (oracle/refcpu.c) -- logits and
 * greedy ids bit-identical to it; slow (one wavefront per output element).  Takes effect with the next evaluation; the KV cache and positions are kept.  0 / 1 */
MINIGPT4_API int minigpt4_amd_set_parity(struct MiniGPT4Context *ctx, int on);
MINIGPT4_API int minigpt4_amd_parity(struct MiniGPT4Context *ctx);                 /* 1 / 0; -1 without a context */

/* ---- measurement ---------------------------------------------------------------------------------------------------- */
/* `steps` greedy decode steps fed back on the device (no host round trip between steps); hipEvent time of steps 1..steps-1. */
MINIGPT4_API int minigpt4_amd_decode_loop(struct MiniGPT4Context *ctx, int steps, int32_t *tokens_out, float *ms_total);
/* hipEvent-bracketed timing of every quantised mat-vec launch over `steps` eager decode steps.
 * out_ms / out_bytes / out_launches are indexed by ggml type id (length 20); other_ms = everything else in the steps. */
MINIGPT4_API int minigpt4_amd_profile_sites(struct MiniGPT4Context *ctx, int steps, char *json_out, size_t capacity);   /* per-launch-site table of `steps` eager decode steps (the captured graph's launch set): JSON, see Engine::profile_sites; 2 = buffer too small */
MINIGPT4_API double minigpt4_amd_weight_bytes_per_token(struct MiniGPT4Context *ctx);
MINIGPT4_API float minigpt4_amd_last_encode_ms(struct MiniGPT4Context *ctx);     /* hipEvent time of the last minigpt4_encode_image */
MINIGPT4_API int minigpt4_amd_sync(struct MiniGPT4Context *ctx);

/* ---- batched image encode (data-parallel requests; carriers from reference minigpt4.h:80-90) --------------------- */
/* Encodes images->n_images images; allocates embeddings->embeddings[i].data like minigpt4_encode_image does. */
MINIGPT4_API int minigpt4_amd_encode_images(struct MiniGPT4Context *ctx, IN const struct MiniGPT4Images *images, OUT struct MiniGPT4Embeddings *embeddings, size_t n_threads);
MINIGPT4_API int minigpt4_amd_free_embeddings(struct MiniGPT4Embeddings *embeddings);
/* DEPRECATED aliases of the two functions above (their names until round 5): they live in the reference's own minigpt4_ namespace and would collide with an upstream
 * implementation of its declared-but-unused MiniGPT4Images API (reference minigpt4.h:80-90).  Forwarders for one more release; new callers use the minigpt4_amd_ names. */
MINIGPT4_API int minigpt4_encode_images(struct MiniGPT4Context *ctx, IN const struct MiniGPT4Images *images, OUT struct MiniGPT4Embeddings *embeddings, size_t n_threads);
MINIGPT4_API int minigpt4_free_embeddings(struct MiniGPT4Embeddings *embeddings);

/* ---- several conversations per context: batched decode ---------------------------------------------------------
 * The reference keeps ONE conversation per context (minigpt4.cpp:2513-2521).  Here a context can own n of them -- each with its own fp16 KV cache region,
 * position and prompt queue, all sharing one copy of the weights.  Every reference entry point (minigpt4_system_prompt, minigpt4_begin_chat(_image),
 * minigpt4_end_chat(_image), minigpt4_reset_chat) acts on the SELECTED conversation (0 after load), so existing callers see no change. */
MINIGPT4_API int minigpt4_amd_set_conversations(struct MiniGPT4Context *ctx, int n);        /* 1..64; reallocates the KV caches and resets every conversation; 0 / 1 */
MINIGPT4_API int minigpt4_amd_select_conversation(struct MiniGPT4Context *ctx, int slot);   /* 0 / 1 (out of range) */
MINIGPT4_API int minigpt4_amd_n_conversations(struct MiniGPT4Context *ctx);
/* One minigpt4_end_chat step for n DISTINCT conversations at once: each is sampled with the given parameters (temp <= 0: greedy) and the n sampled tokens are
 * evaluated in ONE pass over the weights.  tokens[i]: borrowed piece for slots[i], as minigpt4_end_chat returns it.  A conversation whose context is full is
 * sampled but not advanced.  0, or 1 on bad arguments / device error. */
MINIGPT4_API int minigpt4_amd_end_chat_batch(struct MiniGPT4Context *ctx, const int32_t *slots, int n, const char **tokens, float temp, int32_t top_k, float top_p, float tfs_z,
                                             float typical_p, int mirostat, float mirostat_tau, float mirostat_eta);
/* The same step with GIVEN next tokens (teacher forcing): conversation slots[i] is advanced by tokens[i] instead of the token its own logits choose; greedy_out[i] (may be
 * NULL) receives that own greedy choice.  Lets a test / bench leg compare every step's logits of B batched conversations with B independent oracle conversations fed the
 * same ids (reference behaviour: one independent conversation per context, minigpt4.cpp:2513-2521, 2704-2718).  0 / 1. */
MINIGPT4_API int minigpt4_amd_eval_batch(struct MiniGPT4Context *ctx, const int32_t *slots, int n, const int32_t *tokens, int32_t *greedy_out);
/* The queued prompt rows (system prompt, image turn, question...) of n DISTINCT conversations in as few passes over the weights as possible: their rows are packed
 * into chunks of at most n_batch rows, one pass per chunk.  Afterwards each listed conversation is where its own evaluation would have left it (everything queued
 * evaluated, its last-row logits and greedy token current); one with nothing queued is skipped and keeps its logits.  0, or 1 on a bad slot list (duplicates,
 * out of range, n < 1 or n > the number of conversations) or a device error (text in minigpt4_amd_last_error; a failed pass drops the queued rows of every
 * listed conversation, as a failed evaluation of one does). */
MINIGPT4_API int minigpt4_amd_prefill_batch(struct MiniGPT4Context *ctx, const int32_t *slots, int n);
/* Launch kinds of the batched step as last built (eager or at graph capture): out = {rows, k_matvec_ri launches, k_matvec_ri_mix launches, k_matvec_ri launches that split K
 * over workgroups (w2), v_dot4 multi-row launches, v_dot4 mixed-type launches, per-matrix k_mul_mat launches, layers on the int8-MFMA set launches (B >= 5)}.  0 / 1. */
MINIGPT4_API int minigpt4_amd_batch_path(struct MiniGPT4Context *ctx, int32_t out[8]);

/* ---- context shift (llama.cpp's answer to a full context) -------------------------------------------------------------------------------
 * The reference fails every add once n_past + n > n_ctx (FailedToAddString / FailedToAddEmbedding).  A shift keeps the conversation: rows [n_keep, n_keep + n_discard)
 * of the SELECTED conversation are dropped, the rows above slide down in place and their cached keys are re-rotated by -n_discard positions (RoPE is relative).
 * Pending prompt rows are evaluated first, at their current positions.  The last logits stay valid: the next sample uses them.  Shifted keys are rounded to fp16 a
 * second time, so a shifted history is close to, not bit-identical with, one computed at the new positions.
 * minigpt4_amd_shift_context: 0, or 1 (n_keep < 0, n_discard < 0, n_keep + n_discard > n_past; text in minigpt4_amd_last_error) with the conversation untouched.
 * minigpt4_amd_set_context_shift: the automatic policy of this context; n_keep < 0 = off (the default, reference behaviour).  When on, an add that would overflow
 * first shifts by max(n_past + n - n_ctx, (n_past - n_keep) / 2) rows, and minigpt4_amd_end_chat_batch / _eval_batch shift a full conversation and advance it.  An
 * add of more than n_ctx - n_keep rows still fails and shifts nothing.  0 / 1 (no context). */
MINIGPT4_API int minigpt4_amd_shift_context(struct MiniGPT4Context *ctx, int n_keep, int n_discard);
MINIGPT4_API int minigpt4_amd_set_context_shift(struct MiniGPT4Context *ctx, int n_keep);

/* ---- reuse of cached rows: conversation fork and a token-prefix cache -------------------------------------------------------------------------
 * The K / V rows of a causal model depend only on the rows before them, so rows evaluated once can be copied instead of evaluated again (one copy launch for every
 * layer, keys and values, all destinations).  Bit-exact in parity mode; otherwise the rows evaluated after a copied prefix run in a pass of a different size, which moves
 * logits by as much as minigpt4_amd_prefill_batch does against one pass per conversation.
 * minigpt4_amd_fork_conversation: conversation src_slot -> the n_dst DISTINCT other conversations dst_slots.  n_rows = -1: the whole state -- the source's queued rows
 * are evaluated first, then its rows, last logits, greedy token and position are copied; every destination can be sampled at once and continues exactly like the source
 * (k questions about one image: one image turn, fork, k question-only passes).  0 <= n_rows <= n_past(src): that prefix only; the destinations stand at n_past = n_rows
 * WITHOUT current logits, like after minigpt4_reset_chat: add rows before sampling.  Whatever a destination held (rows, queued prompt) is dropped.  0, or 1 with the
 * text "fork_conversation: ..." in minigpt4_amd_last_error and every conversation untouched (a slot out of range, a duplicate, a destination equal to the source,
 * n_dst < 1, n_rows < -1 or > n_past(src)).
 * minigpt4_amd_set_prefix_cache: the prefix cache of this context, off (0) by default.  max_rows > 0 (clamped to n_ctx) allocates ONE stored prefix of up to max_rows
 * rows: 2 * n_layer * max_rows * n_embd * 2 bytes (13B, 256 rows: 210 MB).  A prompt pass that starts at position 0 (minigpt4_end_chat..., minigpt4_amd_get_logits,
 * minigpt4_amd_prefill_batch -- there all matching conversations of the call share one copy launch) compares the leading TOKEN rows of its queue with the stored ids;
 * a common prefix of at least 8 rows is copied instead of evaluated (never the queue's last row: one row is always evaluated, so that logits exist).  After such a
 * pass, a leading token run of at least 8 rows that the store did not cover replaces the store (first max_rows rows; at most one capture per call).  So the constant
 * system prompt + "Human: <Img>" of image turns (the run ends where the image rows begin) is captured once and served to every later request; a text-only chat, whose
 * run is its whole queue, re-captures its own run each time (one copy).  The store is emptied by minigpt4_amd_set_conversations, by a minigpt4_amd_set_parity that
 * changes the mode, and by calling this function again (same value: clear and zero the counters; 0: free it).  0 / 1 (no context, max_rows < 0, out of memory).
 * minigpt4_amd_prefix_cache_info: out = {max_rows, stored_rows, hits, rows_reused_total, captures, rows_reused_by_last_pass (summed over the conversations of the last
 * call that started a pass at position 0), copy launches made by hits (a batched call with 4 hits adds 1)}.  0 / 1. */
MINIGPT4_API int minigpt4_amd_fork_conversation(struct MiniGPT4Context *ctx, int src_slot, const int32_t *dst_slots, int n_dst, int n_rows);
MINIGPT4_API int minigpt4_amd_set_prefix_cache(struct MiniGPT4Context *ctx, int max_rows);
MINIGPT4_API int minigpt4_amd_prefix_cache_info(struct MiniGPT4Context *ctx, int32_t out[7]);

/* ---- scoring: log-probabilities of GIVEN tokens (llama.cpp's logits_all / perplexity) ---------------------------------------------------------
 * The prompt pass keeps one logits row per conversation; these two calls also report what the model thought of every row before it, from the same pass (the output
 * matrix runs on the scored rows in tiles of 64, one more kernel turns each row into numbers) instead of one weight pass per token.
 * minigpt4_amd_score_tokens, on the selected conversation: rows already queued are evaluated first, as their own pass (what minigpt4_amd_get_logits does); then `tokens`
 * are appended and evaluated in chunks of n_batch.  Afterwards position, last logits, greedy token and feed token equal BIT FOR BIT what minigpt4_amd_eval_tokens +
 * minigpt4_amd_get_logits of the same tokens leave: the conversation can be sampled and continued.  Outputs are indexed by the distribution a token is drawn from: entry
 * i describes the distribution that predicts tokens[i] -- for i >= 1 the logits of row i - 1 of this call, for i == 0 the conversation's logits from before the call.
 * logprob_out[i] = log softmax(logits_i)[tokens[i]] (natural logarithm), greedy_out[i] = the argmax of that distribution (first maximum), greedy_logprob_out[i] = its
 * log-probability, logits_out[i] = the row itself.  The logits after tokens[n - 1] are not in logits_out: they are the conversation's current logits
 * (minigpt4_amd_get_logits).  A conversation without current logits (nothing evaluated yet, after minigpt4_reset_chat, after a partial fork) gets logprob 0, greedy -1,
 * greedy_logprob 0 and a zero logits row in entry 0 (llama.cpp's perplexity skips the first token too).  greedy_out, greedy_logprob_out and logits_out may be NULL.
 * Perplexity of a sequence = exp(-mean(logprob_out[1 .. n - 1])).  0, or 1 with the text "score_tokens: ..." in minigpt4_amd_last_error and nothing of `tokens` added (no
 * context, tokens or logprob_out NULL, n < 1, an id outside [0, n_vocab), rows that do not fit n_ctx under minigpt4_amd_eval_tokens' rule, automatic shift included).
 * Score passes neither consult nor fill the prefix cache.
 * minigpt4_amd_score_batch: the same for n_slots DISTINCT conversations -- tokens, counts (each >= 1) and the outputs concatenated in slot-list order.  Queued rows
 * are evaluated first (as minigpt4_amd_prefill_batch(slots) does), then all conversations' tokens run packed, in as few passes as minigpt4_amd_prefill_batch takes; every
 * conversation ends bit-identical to minigpt4_amd_prefill_batch of the same tokens.  After minigpt4_amd_fork_conversation this scores k candidate answers to one image
 * and question for one image turn (multiple-choice evaluation: sum each candidate's entries).  Parity mode: one minigpt4_amd_score_tokens per conversation, in slot order.
 * 0, or 1 with "score_batch: ..." and every conversation untouched (a bad slot list, a count < 1, a bad id, an overflow: all checked before anything runs).  A pass or an
 * automatic shift that fails on the device afterwards returns 1 with the same prefix; what the call had evaluated or shifted by then stays, as after a failed
 * minigpt4_amd_prefill_batch. */
MINIGPT4_API int minigpt4_amd_score_tokens(struct MiniGPT4Context *ctx, const int32_t *tokens, int n, float *logprob_out, int32_t *greedy_out, float *greedy_logprob_out,
                                           float *logits_out);
MINIGPT4_API int minigpt4_amd_score_batch(struct MiniGPT4Context *ctx, const int32_t *slots, int n_slots, const int32_t *tokens, const int32_t *counts, float *logprob_out,
                                          int32_t *greedy_out, float *greedy_logprob_out);

/* ---- top-N alternatives with log-probabilities (the `logprobs=N` of completion APIs, llama.cpp server's n_probs) ------------------------------------------------------
 * One kernel (k_topn_rows, one workgroup per logits row, a constant number of sweeps whatever top_n and the data) selects on the device: a 32001-float row never travels
 * to the host to be sorted.  ORDER: logit descending, equal logits (float equality: -0.0 and +0.0 tie) by ascending token id.  top_n is 1 .. 64 and <= n_vocab.  A
 * log-probability is log softmax(raw logits) (natural logarithm), whatever sampling parameters are in use, and is bit for bit the value minigpt4_amd_score_tokens reports
 * for the same token of the same row.  rank = the number of tokens that sort before a token in that order (0: it is the greedy token).  Every call returns 0, or 1 with
 * a text in minigpt4_amd_last_error that begins with the call's short name ("top_logprobs: ...") -- and on a refusal of its arguments nothing has changed.
 * minigpt4_amd_token_piece: the borrowed text of a token id, as minigpt4_end_chat returns it ("</s>" for id 2); NULL without a context or for an id outside [0, n_vocab).
 * minigpt4_amd_top_logprobs: what each of n_slots DISTINCT conversations would say next, without advancing anything.  Queued rows are evaluated first, exactly as
 * minigpt4_amd_prefill_batch(ctx, slots, n_slots) does; then one launch over the listed conversations' logits, one copy back, one synchronise.  top_ids_out /
 * top_logprobs_out: [n_slots][top_n].  targets (may be NULL; an entry of -1 = none): logprob_out[i] / rank_out[i] (each may be NULL) describe targets[i] (none: 0 / -1).
 * A conversation without current logits (nothing evaluated, after minigpt4_reset_chat, after a partial fork): ids -1, log-probabilities 0, rank -1.  Position, logits,
 * greedy token, feed token, the sampler's generator and the mirostat state are untouched.  Refused: no context, a bad slot list, NULL top_ids_out / top_logprobs_out,
 * top_n out of range, a target outside [-1, n_vocab).
 * minigpt4_amd_end_chat_batch_top: minigpt4_amd_end_chat_batch that also reports, for EVERY listed conversation (one that is full, sampled but not advanced, included),
 * the sampled id (ids_out[n]), its log-probability and rank (logprob_out[n], rank_out[n]) and the top_n alternatives of the distribution it was drawn from
 * (top_ids_out / top_logprobs_out [n][top_n]).  Conversations, pieces and sampler draws are exactly minigpt4_amd_end_chat_batch's in the same state; the kernel runs
 * between the sampling and the weight pass and its results are awaited while the pass runs.  All five outputs are required.
 * minigpt4_amd_score_tokens_top: minigpt4_amd_score_tokens with rank_out[n] and the alternatives top_ids_out / top_logprobs_out [n][top_n] of every entry (same entry
 * indexing; column 0 is score_tokens' greedy / greedy_logprob).  Entry 0 of a conversation without logits: logprob 0, rank -1, ids -1, log-probabilities 0.  logprob_out
 * and the conversation afterwards are bit for bit what minigpt4_amd_score_tokens of the same tokens gives.  All four outputs are required.  The result arrays of the
 * feature are allocated by the first of these calls: plain scoring and plain decoding pay nothing and launch nothing new.
 * Not built: a packed minigpt4_amd_score_batch with alternatives; log-probabilities of tempered or filtered distributions; any use of the selection by the sampler
 * (minigpt4_amd_beam_search below is the one consumer of the selection on the device). */
MINIGPT4_API const char *minigpt4_amd_token_piece(struct MiniGPT4Context *ctx, int32_t id);
MINIGPT4_API int minigpt4_amd_top_logprobs(struct MiniGPT4Context *ctx, const int32_t *slots, int n_slots, int top_n, const int32_t *targets, int32_t *top_ids_out,
                                           float *top_logprobs_out, float *logprob_out, int32_t *rank_out);
MINIGPT4_API int minigpt4_amd_end_chat_batch_top(struct MiniGPT4Context *ctx, const int32_t *slots, int n, const char **tokens, float temp, int32_t top_k, float top_p, float tfs_z,
                                                 float typical_p, int mirostat, float mirostat_tau, float mirostat_eta, int top_n, int32_t *ids_out, float *logprob_out,
                                                 int32_t *rank_out, int32_t *top_ids_out, float *top_logprobs_out);
MINIGPT4_API int minigpt4_amd_score_tokens_top(struct MiniGPT4Context *ctx, const int32_t *tokens, int n, int top_n, float *logprob_out, int32_t *rank_out, int32_t *top_ids_out,
                                               float *top_logprobs_out);

/* ---- speculation: draft tokens verified in one weight pass; greedy lookup decoding (llama.cpp's lookup example, the `draft` family of its server) ------------------
 * A decode step streams every weight for ONE row.  A caller who can guess the next few tokens -- from the prompt, from a smaller model in a second context, from a
 * template -- lets the conversation put its next token AND the guesses through one pass (the batched step's mat-vec launches at 1 + n rows, an attention launch that is
 * causal among the rows, an epilogue that decides on the device how many rows count) and keeps the guesses the pass's own logits confirm: under greedy decoding the
 * tokens are exactly those plain decoding emits, 1 + m of them for one pass.  Each call returns 0, or 1 with "<short name>: ..." in minigpt4_amd_last_error; on a
 * refusal of its arguments nothing has changed.
 * minigpt4_amd_set_speculation: off (0) by default; max_draft 1 .. 7 allocates 1 + max_draft logits rows, a small result block and one captured pass per row count (at
 * first use); 0 frees them.  Plain decoding, batched decoding and scoring pay nothing and launch nothing new either way.  At 3 and 4 rows the pass runs on the
 * row-interleaved int8-MFMA image of the k-quant weights where the context already HAS it (minigpt4_amd_set_conversations(n > 1) builds it; it doubles those weights'
 * memory): this call never builds it.  The setting survives minigpt4_amd_set_parity and minigpt4_amd_set_conversations; the captured passes are dropped there.
 * Refused (1, "set_speculation: ...", nothing allocated, the setting stays off): max_draft > 0 on a context whose n_ctx exceeds what the verify pass's attention kernel
 * holds in LDS -- it keeps 8 new key / value rows there where the decode step keeps one: 23 792 rows at head size 128 (the load admits 24 392), 24 160 at 64 (24 456), 24 336 at 32 (24 488).
 * minigpt4_amd_verify_draft, on the selected conversation: queued rows are evaluated first (as minigpt4_amd_get_logits does); the conversation must then have current
 * logits.  g0 = its greedy token (what minigpt4_end_chat at temp 0 would emit).  ONE pass evaluates g0, draft[0 .. n_draft) at positions p, p + 1, ...; g[r + 1] = the
 * first argmax of row r; m = the largest value with draft[i] == g[i + 1] for all i < m.  Afterwards ids_out[0 .. m] = g0, draft[0 .. m - 1], *n_out = 1 + m, the
 * conversation stands at n_past = p + 1 + m with the logits, greedy token and feed token of row m, and can be sampled, scored, forked or shifted as after any
 * evaluation.  (Cache rows above n_past hold the rejected rows: dead -- a fork copies n_past rows, the next evaluation overwrites them.)  row_greedy_out (may be NULL;
 * 1 + n_draft entries) = g[1 ...] of every evaluated row, -1 for a row that was not evaluated.  n_draft = 0 is one greedy step.  A draft longer than the room left is
 * cut to n_ctx - n_past - 1 rows; with no room for g0 the call follows minigpt4_amd_eval_tokens' rule: the automatic shift makes room, else 1 with "verify_draft:
 * context full".  Refused: no context, speculation off, n_draft < 0 or > max_draft, draft NULL with n_draft > 0, ids_out / n_out NULL, an id outside [0, n_vocab), no
 * current logits.  The sampler's generator, the mirostat state and the prefix cache are untouched.  Parity mode: one single-row oracle-order pass per row, stopping at
 * the first mismatch -- bit-identical to plain greedy decoding, no speed-up (as minigpt4_amd_score_batch and the batched step fall back).  No key-split attention:
 * the pass's attention is the one-workgroup-per-head form at any context length.
 * minigpt4_amd_decode_lookup: the greedy generation loop with an n-gram drafter on the host.  History = corpus (may be empty) followed by what this call has emitted.
 * Before each pass: the longest suffix of the history (ngram_max down to ngram_min tokens, ending in the token about to be evaluated) that occurs earlier, the most
 * recent occurrence among equals; the draft = the tokens that followed it, cut at n_draft (1 .. max_draft), before any id 2 and at the tokens still wanted.  No match:
 * the ordinary decode step of minigpt4_end_chat at temp 0 (its own graph, key-split attention at long contexts) -- text the drafter cannot guess costs what it costs
 * today.  Ends after max_tokens, after emitting and evaluating </s>, or when the context is full and cannot shift.  tokens_out[max_tokens], *n_tokens;
 * stats = {verify passes, plain steps, draft tokens sent, draft tokens accepted} (passes + steps + accepted == *n_tokens).
 * WHICH n_draft: NOT MEASURED YET.  A pass of R = 1 + n_draft rows pays when the draft tokens it keeps per pass exceed pass_ms / plain_step_ms - 1; tools/lookup_decode.py
 * prints that break-even per R (its table c) next to the pass and step times it follows from.  Until its log is recorded the only figure is the batched step's: four rows
 * per pass cost 3.87 ms against 2.65 ms for one -- about 0.46 kept draft tokens of 3 to break even -- which is why the loop never drafts without a match. */
MINIGPT4_API int minigpt4_amd_set_speculation(struct MiniGPT4Context *ctx, int max_draft);
MINIGPT4_API int minigpt4_amd_verify_draft(struct MiniGPT4Context *ctx, const int32_t *draft, int n_draft, int32_t *ids_out, int32_t *n_out, int32_t *row_greedy_out);
MINIGPT4_API int minigpt4_amd_decode_lookup(struct MiniGPT4Context *ctx, const int32_t *corpus, int n_corpus, int max_tokens, int ngram_max, int ngram_min, int n_draft,
                                            int32_t *tokens_out, int32_t *n_tokens, int32_t stats[4]);

/* ---- repetition, frequency and presence penalties; logit bias (llama.cpp master-31cfbb1: llama_sample_repetition_penalty, llama_sample_frequency_and_presence_penalties,
 * applied in the order of llama.cpp's main) ------------------------------------------------------------------------------------------------------------------------------
 * The reference accepts repeat_last_n, repeat_penalty, alpha_presence, alpha_frequency and penalize_nl in minigpt4_end_chat(_image) and ignores them.  So does this library
 * BY DEFAULT (bit-compatibility); the mode below is an opt-in.
 * NEUTRAL VALUES ARE repeat_penalty 1.0, alpha_presence 0.0, alpha_frequency 0.0.  THE REFERENCE BINDING'S DEFAULTS FOR THE TWO ALPHAS ARE 1.0: a caller who switches the
 * mode on and keeps those defaults gets a frequency penalty of 1 per occurrence plus a presence penalty of 1 on every token of the window.
 * HISTORY.  Every conversation keeps a row-aligned token history: entry r is the token id of cache row r, or -1 for a row that came in as an embedding (the 32 image rows,
 * minigpt4_amd_eval_embd).  Prompt passes, batched steps (forced ids included), scoring, draft verification (kept rows only), forks (whole or prefix copy), prefix-cache hits
 * all keep it in step; minigpt4_reset_chat and minigpt4_amd_set_conversations clear it (set_conversations also resets parameters and bias); a context shift REMOVES the
 * shifted rows from it.  minigpt4_amd_decode_loop and minigpt4_amd_profile_sites feed tokens back on the device and are measurement entry points: their rows enter as -1.
 * Rows that are queued but not evaluated count, because sampling evaluates them first.
 * WINDOW.  The last min(len(history), W) entries, W = n_ctx if repeat_last_n < 0, else repeat_last_n, clamped to 1024.  A -1 entry takes a place in the window and
 * penalises nothing.  count[id] = occurrences of id in the window.
 * ARITHMETIC on a copy of the logits row l, every operation rounded to fp32 on its own (no fused multiply-add):
 *   1. l[id] += bias[id] for each bias pair;   2. nl = l[13] (13 = llama_token_nl(); skipped when n_vocab <= 13);
 *   3. window non-empty and repeat_penalty != 1: for every id with count > 0, l = (l <= 0) ? l * repeat_penalty : l / repeat_penalty;
 *   4. window non-empty and not both alphas 0: for every id with count > 0, t = float(count) * alpha_frequency; t = t + alpha_presence; l = l - t;
 *   5. !penalize_nl: l[13] = nl (the value AFTER the bias).
 * With temp <= 0 the pick is the FIRST maximum of the result (lowest id among equal values, -0.0 == +0.0), found by one kernel launch (k_pen_pick) over all listed
 * conversations of the call -- no logits row travels to the host; with temp > 0 the result feeds the sampling chain (top-k, mirostat, ... see penalised logits, as in
 * llama.cpp).  Host and device share one definition of the arithmetic and agree bit for bit; parity mode changes nothing here: the transformation is exact and the same.
 * The logits themselves are never modified: minigpt4_amd_get_logits, the scoring calls, minigpt4_amd_top_logprobs and the report of minigpt4_amd_end_chat_batch_top keep
 * describing the RAW distribution (a log-probability is that of the raw logits, as promised above).
 * minigpt4_amd_verify_draft, minigpt4_amd_decode_lookup and minigpt4_amd_decode_loop decide on raw logits and ignore penalties and bias; their tokens still enter the history.
 * A conversation whose transformation is the identity (neutral parameters or an empty window, and no bias) takes exactly the path it takes with the mode off: no launch,
 * no copy, no allocation.  The feature's buffers are allocated by its first launch.
 * minigpt4_amd_set_penalties: on = 0 (default; also MINIGPT4_PENALTIES=1 in the environment at load switches it on, for the reference's unmodified binding and web UI): the
 * five arguments are ignored.  on = 1: minigpt4_end_chat(_image) first stores its five arguments as the selected conversation's parameters (arguments that
 * minigpt4_amd_conversation_penalties would refuse are not stored; minigpt4_amd_last_error says so), then samples with them.  Returns 0, or 1 without a context.
 * minigpt4_amd_conversation_penalties: stores a conversation's parameters (default: 64, 1.0, 0.0, 0.0, 1); they take effect only while the mode is on.
 * minigpt4_amd_end_chat_batch, minigpt4_amd_end_chat_batch_top and minigpt4_amd_sample have no penalty arguments and use each conversation's stored parameters.  Refused
 * (1, "conversation_penalties: ...", nothing changed): a slot out of range, repeat_penalty <= 0 or not finite, an alpha that is not finite.
 * minigpt4_amd_set_logit_bias: the selected conversation's bias, at most 256 (id, bias) pairs, n = 0 clears it; active WHATEVER the mode; -INFINITY bans a token.  It
 * survives minigpt4_reset_chat.  Refused (1, "set_logit_bias: ...", nothing changed): NaN or +INFINITY, an id outside [0, n_vocab), a duplicate id, n < 0 or > 256.
 * minigpt4_amd_token_history: evaluates the selected conversation's queued rows, writes the first min(count, cap) entries of its history to out (may be NULL) and returns
 * the count (-1: no context, or the pass failed).
 * minigpt4_amd_penalty_info: out = {mode, k_pen_pick launches so far, rows penalised on the host so far, table entries uploaded by the last launch}. */
MINIGPT4_API int minigpt4_amd_set_penalties(struct MiniGPT4Context *ctx, int on);
MINIGPT4_API int minigpt4_amd_conversation_penalties(struct MiniGPT4Context *ctx, int slot, int32_t repeat_last_n, float repeat_penalty, float alpha_presence,
                                                     float alpha_frequency, int penalize_nl);
MINIGPT4_API int minigpt4_amd_set_logit_bias(struct MiniGPT4Context *ctx, const int32_t *ids, const float *bias, int n);
MINIGPT4_API int minigpt4_amd_token_history(struct MiniGPT4Context *ctx, int32_t *out, int cap);
MINIGPT4_API int minigpt4_amd_penalty_info(struct MiniGPT4Context *ctx, int32_t out[4]);

/* ---- beam search over forked conversations, selected on the device (the "beam search numbers" of MiniGPT-4's demo, llama.cpp's llama_beam_search) ----------------------
 * Every other generation entry point follows ONE hypothesis per conversation.  This call keeps n_beams of them, each in a conversation of its own, and puts all of them
 * through ONE weight pass per step (the batched step of minigpt4_amd_eval_batch at n_beams rows -- the same launches, no new mat-vec or attention code).  Between the logits
 * of one step and the pass of the next there is no host round trip: k_topn_rows lists every beam's best tokens, k_beam_select picks the n_beams best (beam, token) pairs and
 * writes the next pass's row tokens, k_kv_permute makes beam i continue from its parent's cache rows (any map -- swaps, cycles, all-to-one -- in one launch); the host reads
 * a 44-word result block per step through pinned memory while the pass runs.
 * slots: n_beams DISTINCT conversations, 2 <= n_beams <= 8; slots[0] is the SOURCE, the others are scratch.  The source's queued rows are evaluated first (as
 * minigpt4_amd_get_logits does); it must then have current logits.  Its logits row is saved and its state forked to the other slots.
 * THE RULE, W = n_beams, C = 2 W, EOS = id 2 ("</s>"), fp32 throughout.  A live beam i carries the cumulative score s[i]; step t (t = 0, 1, ...: t tokens emitted so far)
 * takes each beam's C best tokens in k_topn_rows' order (logit descending, equal logits by ascending id) with their log-probabilities lp[i][c] (log softmax of the RAW
 * logits, bit for bit minigpt4_amd_top_logprobs' values).  Candidate (i, c) scores s[i] + lp[i][c] (one add, no fused multiply-add).  The W C candidates are ranked by score
 * descending; equal scores (float equality: -0 and +0 tie) by ascending beam, then ascending c.  The ranking is walked from the top: an EOS candidate at a rank below W
 * FINISHES a hypothesis -- tokens = the beam's tokens + EOS, final score = score / powf((float)(t + 1), length_penalty) --, an EOS candidate at rank W or above is skipped,
 * any other candidate becomes the next live beam, in walk order, until W are filled (a beam lists EOS at most once, so C = 2 W always fills them).  In step 0 only beam 0
 * is live (the others score -INFINITY and their candidates are ignored): its C best tokens fill all W beams.  The search ENDS after the step that brings the finished list
 * to at least W hypotheses (the list keeps the W best under the order below and drops the rest), or after max_tokens steps; then the live beams join the list UNFINISHED:
 * score / powf((float)steps, length_penalty) with the steps that ran (max_tokens, or the room), no EOS appended.  RESULT ORDER: final score descending; equal scores: finished before unfinished, then earlier creation
 * first (walk order, step after step; the unfinished ones in beam order).  length_penalty 0 compares raw sums, 1 the mean log-probability.
 * Outputs: *n_out = min(n_best, hypotheses) rows; tokens_out is [n_best][max_tokens + 1] (-1 behind a row's length), lengths_out / scores_out [n_best].  stats = {weight
 * passes (= steps: the step that ends the search still runs its pass), k_kv_permute launches whose map was not the identity, cache rows moved (rows x conversations that
 * took another beam's rows; the launch covers only the rows that can differ between the beams: from the last step whose beams all had one parent on), hypotheses finished
 * by EOS}.
 * AFTERWARDS slots[0] is bit for bit what it was -- position, logits, greedy token, feed token, token history -- and the other slots stand as
 * minigpt4_amd_fork_conversation(n_rows = that position) leaves them; continue the chat with minigpt4_amd_eval_tokens(best hypothesis).  Cache rows above the position are
 * dead, as after minigpt4_amd_verify_draft.  The search needs max_tokens rows of room in every slot: with less, max_tokens is cut to the room; with none the call returns 1
 * with "beam_search: context full".  It never shifts a context.  Decisions are on raw logits: penalties and logit bias are ignored (as in minigpt4_amd_verify_draft); the
 * sampler's generator, the mirostat state and the prefix cache are untouched and no token-history entry survives the call.
 * Parity mode: the same rule and kernels decide; one oracle-order single-row pass per beam and step evaluates (the fall-back of minigpt4_amd_eval_batch).
 * Returns 0, or 1 with "beam_search: ..." in minigpt4_amd_last_error and nothing changed: no context, a bad slot list, n_beams outside 2 .. 8, n_best outside 1 .. n_beams,
 * max_tokens < 1, a length_penalty that is not finite, a NULL output, no current logits, n_vocab <= 2 * n_beams.  The buffers of the feature are allocated by the first
 * call and freed with the context and by minigpt4_amd_set_conversations: a context that never calls it allocates nothing new and launches nothing new.
 * Not built: sampling or diverse beam search, penalties inside the search, more than 8 beams, a device-resident loop without the per-step read-back. */
MINIGPT4_API int minigpt4_amd_beam_search(struct MiniGPT4Context *ctx, const int32_t *slots, int n_beams, int max_tokens, float length_penalty, int n_best, int32_t *tokens_out,
                                          int32_t *lengths_out, float *scores_out, int32_t *n_out, int32_t stats[4]);

/* ---- guided decoding: two conversations' logits contrasted on the device (classifier-free guidance: llama.cpp's llama_sample_classifier_free_guidance behind
 * --cfg-negative-prompt / --cfg-scale; for a vision-language model also image-contrastive decoding: the conversation that saw the image against the same question
 * without it) ------------------------------------------------------------------------------------------------------------------------------------------------------
 * Every other generation entry point decides a token from ONE conversation's logits.  Here a PAIR decides: a guided conversation pos = slots[i] and a guidance
 * conversation neg = neg_slots[i], all 2 n of a call distinct conversations of one context, 1 <= n <= 32.  b and g are their current RAW logits rows, scale a finite
 * float: 1 = no guidance, above 1 pushes away from neg, 0 and negative values are allowed.
 * THE RULE, fp32 throughout:
 *   1. lb[j] = (b[j] - max b) - log(sum exp(b - max b)), lg likewise from g: bit for bit the log-probabilities minigpt4_amd_top_logprobs reports for those rows.
 *   2. d = lb[j] - lg[j];  t = scale * d;  m[j] = lg[j] + t -- each operation rounded to fp32 on its own, no fused multiply-add (llama.cpp's
 *      l = guidance + scale * (base - guidance) on the two log-softmaxed rows).  Exactly: scale == 0 gives m == lg, and b, g being one row gives m == lb.
 *   3. m is what everything downstream of the logits sees for pos, in the order of llama.cpp's main: guidance, then pos's logit bias and penalties (steps 1 - 5 above,
 *      applied to m), then the pick.  neg's bias and penalties are ignored.
 *   4. temp <= 0: the first maximum of the result (lowest id among equal values, -0.0 == +0.0).  temp > 0: the sampling chain on the result, one draw per pair, in list order.
 *   5. BOTH conversations advance by the picked token in one weight pass -- the batched step's own launches and graph; the token enters both token histories.  Afterwards
 *      each holds its own raw logits, greedy token and feed token, bit for bit as after minigpt4_amd_eval_batch with that token forced on both.
 *   6. A pair advances both conversations or neither: if either has no room and the automatic shift (minigpt4_amd_set_context_shift) cannot make it, the pair is sampled, its
 *      id reported, and neither advances.  With the shift on each conversation shifts by its own rule.
 * Logits are finite (NaN and infinities in the raw rows: unspecified).  The raw rows are never modified: minigpt4_amd_get_logits, the scoring calls and
 * minigpt4_amd_top_logprobs keep describing raw distributions; minigpt4_amd_verify_draft, minigpt4_amd_decode_lookup and minigpt4_amd_beam_search keep deciding on them.
 * ON THE DEVICE: k_guide_rows (one 256-thread workgroup per pair, one launch per call) sweeps the two rows for their maxima and sums, mixes in one more sweep and carries
 * the first maximum.  With temp <= 0 a pair whose pos has no bias and no active penalty never meets the host between the decision and the pass: the kernel writes the pick
 * into the pass's row tokens, and the host reads the ids from pinned memory while the pass runs (it needs them for histories, pieces and ids_out only).  A pair with a bias or
 * penalty runs k_pen_pick on its written m row; with temp > 0 the m rows of all pairs come to the host in one copy.  Parity mode: the same kernel decides, one oracle-order
 * single-row pass per conversation evaluates (the fall-back of minigpt4_amd_eval_batch).
 * Queued rows of all 2 n conversations are evaluated first (as minigpt4_amd_prefill_batch over them does); each must then have current logits.
 * minigpt4_amd_end_chat_guided: one step.  tokens[i] = the borrowed piece of pair i's token (as minigpt4_amd_end_chat_batch returns it), ids_out (may be NULL) its id.
 * minigpt4_amd_guided_logits: mixed_out (may be NULL) = [n][n_vocab] rows m BEFORE bias and penalties, pick_out (may be NULL) their first maxima.  It advances nothing:
 * position, logits, greedy / feed token, the sampler's generator, mirostat state and histories are untouched; only queued rows are evaluated.
 * minigpt4_amd_guidance_info: out = {k_guide_rows launches, pairs handed to the pass on the device, pairs picked through k_pen_pick, pairs sampled on the host} so far.
 * Each returns 0, or 1 with "end_chat_guided: ..." / "guided_logits: ..." / "guidance_info: ..." in minigpt4_amd_last_error and nothing changed: no context, a NULL list,
 * n < 1, 2 n above the number of conversations, a slot out of range or named twice, a scale that is not finite; after the queued rows: "... has no current logits" (after
 * minigpt4_reset_chat, after a partial fork).  The buffers of the feature (32 mixed rows, the tables, an event) are allocated by the first call and freed with the context
 * and by minigpt4_amd_set_conversations: a context that never calls it allocates nothing new and launches nothing new.
 * Not built: a stored pairing that would make the reference's minigpt4_end_chat guided; guidance inside beam search or draft verification; a top-N report of the guided
 * distribution; a smoothing factor; more than 32 pairs. */
MINIGPT4_API int minigpt4_amd_end_chat_guided(struct MiniGPT4Context *ctx, const int32_t *slots, const int32_t *neg_slots, int n, float scale, const char **tokens, float temp,
                                              int32_t top_k, float top_p, float tfs_z, float typical_p, int mirostat, float mirostat_tau, float mirostat_eta, int32_t *ids_out);
MINIGPT4_API int minigpt4_amd_guided_logits(struct MiniGPT4Context *ctx, const int32_t *slots, const int32_t *neg_slots, int n, float scale, float *mixed_out, int32_t *pick_out);
MINIGPT4_API int minigpt4_amd_guidance_info(struct MiniGPT4Context *ctx, int32_t out[4]);

/* ---- constrained decoding: a regular expression per conversation, enforced on the device ------------------------------------------------------------
 * The text a constrained conversation generates -- the bytes of its picked tokens, concatenated -- is kept inside a pattern, and "</s>" is allowed exactly where the text so
 * far matches the WHOLE pattern.  The pattern is compiled once to a byte-level DFA of at most 1024 states (0 = dead, 1 = start); one kernel then builds, for every state,
 * the bitmap of token ids that may follow (k_constrain_index), and a greedy step costs one small launch that takes the first maximum of the transformed logits row over
 * the allowed ids (k_constrain_pick).
 * Pattern syntax (bytes, UTF-8): a literal byte;  .  (any byte except 0x0A);  [...] and [^...] with ranges, a ']' in first place a literal, escapes allowed inside, a byte
 * >= 0x80 inside refused (write \xHH);  ( ) and (?: ), both without capture;  |  with empty alternatives;  * + ? {m} {m,} {m,n} with 0 <= m <= n <= 255 (they stack: a**);
 * \d \w \s \D \W \S (ASCII; the negations range over all 256 bytes), \n \t \r \f \v \0 \xHH, \ + ASCII punctuation = that byte.  A multi-byte UTF-8 character outside a
 * class is its byte sequence and a quantifier behind it applies to the whole character; '.' and negated classes match ONE BYTE.  Refused, with the byte offset: anchors,
 * lazy and possessive quantifiers, back-references, look-around and every other (? group, \ + any other letter or digit, a bare quantifier, groups nested deeper than
 * 250.  Also refused: a pattern longer than 4096 bytes, "too many states" (more than 16 384 positions after the counted repeats are expanded, more than 8192 subsets,
 * more than 1024 states of the minimal automaton), "matches nothing".
 * Constraints belong to the CONTEXT, at most 8 at a time (handles 1 .. 8); they depend on the vocabulary only and survive minigpt4_amd_set_conversations and parity switches.
 * minigpt4_amd_constraint_compile: n_bytes = -1 takes strlen(pattern).  Compiles, uploads, builds the index and synchronises.
 * minigpt4_amd_constraint_free: refused while a conversation uses the handle.
 * minigpt4_amd_set_constraint: handle 0 clears; the conversation's state always goes to the start.  The assignment survives minigpt4_reset_chat (which returns the state to
 * the start), like the logit bias; minigpt4_amd_set_conversations clears it; a fork touches neither handle nor state of any conversation.
 * minigpt4_amd_constraint_advance: walks the state over n token ids on the host, for callers who feed tokens themselves; id 2 ("</s>") leaves the state where it is; a
 * token that leads to the dead state refuses the whole call and changes nothing.
 * minigpt4_amd_constraint_info: out = {handle, state, 1 if the state accepts, states of the automaton, k_constrain_pick launches, rows masked on the host for the sampling
 * chain, picks that found no allowed id, k_constrain_index launches}; the last four count over the context.
 * minigpt4_amd_constraint_mask: out[n_words] <- the device index row of (handle, state): bit i of word i / 32 = token i is allowed.  n_words must be at least
 * (n_vocab + 31) / 32 rounded up to a multiple of 4.  Bits: an id >= 3 whose piece is not empty and whose bytes do not lead to the dead state; id 2 iff the state accepts;
 * never ids 0 and 1.
 * Where it acts: minigpt4_end_chat(_image), minigpt4_amd_sample, minigpt4_amd_end_chat_batch and _end_chat_batch_top, in llama.cpp's order: logit bias, penalties,
 * constraint, then the pick or the chain.  temp <= 0: ONE k_constrain_pick launch over the constrained conversations of the call -- it applies their penalty tables itself,
 * so k_pen_pick skips them --, 4 bytes per conversation come back.  The pick is the FIRST maximum over the allowed ids (lowest id among equal values, -0 == +0); a state
 * without an allowed id picks "</s>" and counts as stuck (a vocabulary with all 256 byte tokens never gets there).  temp > 0: the state's index row comes to the host and
 * every other id of the chain's copy of the row becomes -infinity.  The state belongs to the sampler, like the generator: every constrained pick -- minigpt4_amd_sample's
 * included -- advances it by the picked token, whether or not the conversation then has room to advance.  Parity mode changes nothing: the decision is exact either way.
 * What stays raw: minigpt4_amd_get_logits, scoring, minigpt4_amd_top_logprobs and the _top report describe raw logits; minigpt4_amd_eval_batch neither consults nor
 * advances a constraint.  A conversation without a constraint takes exactly the path it took before: no launch, no copy, no allocation (the vocabulary on the device, the
 * staging and the indices are allocated by the first compile and freed with the context).
 * Each call returns 0, or 1 with "<short name>: ..." in minigpt4_amd_last_error and nothing changed.
 * Not built: minigpt4_amd_end_chat_guided, minigpt4_amd_verify_draft, minigpt4_amd_decode_lookup, minigpt4_amd_beam_search and minigpt4_amd_decode_loop neither consult
 * nor advance a constraint; context-free grammars and JSON-schema translation; character-level '.' and negated classes; handing the constrained pick to the weight pass
 * without the host visit. */
MINIGPT4_API int minigpt4_amd_constraint_compile(struct MiniGPT4Context *ctx, const char *pattern, int n_bytes, int32_t *handle);
MINIGPT4_API int minigpt4_amd_constraint_free(struct MiniGPT4Context *ctx, int32_t handle);
MINIGPT4_API int minigpt4_amd_set_constraint(struct MiniGPT4Context *ctx, int slot, int32_t handle);
MINIGPT4_API int minigpt4_amd_constraint_advance(struct MiniGPT4Context *ctx, int slot, const int32_t *tokens, int n);
MINIGPT4_API int minigpt4_amd_constraint_info(struct MiniGPT4Context *ctx, int slot, int32_t out[8]);
MINIGPT4_API int minigpt4_amd_constraint_mask(struct MiniGPT4Context *ctx, int32_t handle, int state, uint32_t *out, int n_words);

/* ---- sampled batched steps decided on the device, one seed per conversation ------------------------------------------------------------------------------
 * minigpt4_amd_end_chat_batch with temp > 0 samples on the host: one logits row, one synchronise and one sort per listed conversation, all draws from the context's one
 * generator in list order -- so the text a conversation receives depends on who shares its step.  Here ONE launch (k_sample_rows, one 256-thread workgroup per listed
 * conversation) decides the whole step, and every conversation draws from a stream of its own.
 * GENERATOR: Philox4x32-10 (Random123; multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85).  Every conversation has a 64-bit seed and a 64-bit
 * count of draws: key = (seed low word, seed high word), counter = (draws low, draws high, 0, 0), the draw uses output word 0.  After minigpt4_model_load and after
 * minigpt4_amd_set_conversations conversation s has seed = (uint32_t)load seed | (uint64_t)s << 32 and draws = 0.  minigpt4_reset_chat, forks, shifts and snapshot loads
 * touch neither: the pair belongs to the sampler, as the host generator does (the snapshot format does not carry it: set it again with minigpt4_amd_conversation_seed).
 * THE ROW the rule sees is the conversation's raw logits row after the transformations above, in their order: logit bias and penalties (steps 1 - 5), then the
 * conversation's constraint -- only ids allowed in its state take part.  The raw row is never written.
 * CANDIDATES: the first n_c = min(top_k, participating ids) of them in minigpt4_amd_top_logprobs' order (value descending, equal values -- float equality, -0.0 == +0.0 --
 * by ascending id), values v_0 >= v_1 >= ...  No participating id: the pick is "</s>" (id 2), flagged stuck, as the greedy constrained pick; a draw is still counted.
 * THE RULE, fp32 throughout, each operation rounded on its own, no fused multiply-add, sums in candidate order -- llama.cpp's top-k -> top-p -> temperature -> softmax
 * -> draw, the chain of minigpt4_end_chat with tail-free and typical sampling neutral:
 *   1. top_p < 1: a_j = expf(v_j - v_0), A = sum a_j, q_j = a_j / A, c += q_j; kept = the first j + 1 with c >= top_p, n_c if there is none.  top_p == 1: kept = n_c.
 *   2. w_j = v_j / temp for j < kept.
 *   3. b_j = expf(w_j - w_0), S_j the running sum, S = S_{kept - 1}; the reported probability is p_j = b_j / S.
 *   4. u = (float)(word >> 8) * 2^-24, t = u * S, pick = the first j with S_j > t; kept - 1 if there is none (u * S can round up to S).
 *   5. draws += 1, exactly once per decision, also when the conversation then has no room to advance.
 * minigpt4_amd_end_chat_batch_sampled: one minigpt4_amd_end_chat_batch step decided this way.  Queued rows of the listed conversations are evaluated first; each must then
 * have current logits.  Then one descriptor upload, the one launch -- it writes each pick straight into the row tokens of the weight pass --, one small copy of the picks
 * to pinned memory, and the batched step's own pass; the host reads the picks while the pass runs, for histories, constraint states, pieces and ids_out.  No logits row
 * travels to the host and the host does not synchronise between the decision and the pass.  A conversation that is full and cannot shift is sampled and reported but not
 * advanced.  Afterwards every conversation that advanced holds its raw logits, greedy and feed token bit for bit as after minigpt4_amd_eval_batch with the picked tokens
 * forced.  tokens[i] = the borrowed piece of slots[i]'s token, ids_out (may be NULL) its id.  Parity mode: the same kernel decides, one oracle-order single-row pass per
 * conversation evaluates.
 * minigpt4_amd_sampled_candidates: the distribution the next such step would draw from: ids_out [n][64] (-1 behind n_cand), probs_out [n][64] = p_j (0 behind kept),
 * n_cand_out [n], kept_out [n]; each may be NULL.  Only queued rows are evaluated; nothing advances and no draw is counted.
 * minigpt4_amd_conversation_seed: sets both fields of one conversation; setting draws lets a caller resume a stream where it stopped.
 * minigpt4_amd_sampling_info: out = {seed, draws, k_sample_rows launches, picks handed to a pass on the device, picks flagged stuck, rows sampled this way}; the last four
 * count over the context.
 * Each returns 0, or 1 with "end_chat_batch_sampled: ..." / "sampled_candidates: ..." / "conversation_seed: ..." / "sampling_info: ..." in minigpt4_amd_last_error and
 * nothing changed: no context, a NULL or empty list, more entries than conversations, a slot out of range or named twice, temp not finite or <= 0, top_k outside
 * 1 .. min(64, n_vocab), top_p outside (0, 1] (NaN included), tokens NULL; after the queued rows: "... has no current logits".  A pick outside the vocabulary read back
 * from the device is an error after the fact, reported as minigpt4_amd_end_chat_guided reports it.
 * What stays as it was: minigpt4_amd_end_chat_batch and _end_chat_batch_top, minigpt4_end_chat(_image), minigpt4_amd_sample and minigpt4_amd_end_chat_guided keep the host
 * chain and the context's generator; their draws neither read nor move a conversation's (seed, draws).  The buffers of the feature (descriptors, result block, pinned
 * mirror, an event) are allocated by the first call and freed with the context and by minigpt4_amd_set_conversations: a context that never calls these functions
 * allocates nothing new and launches nothing new.
 * Tail-free, typical and min-p filters and mirostat v2: the extended rule below (the _ex calls).
 * Not built: mirostat v1; mirostat over the whole vocabulary; top_k = 0 or above 64; mu in snapshots; a top-N report of the sampled step; guided sampling on the device; a
 * mode that redirects the reference's minigpt4_end_chat here. */
MINIGPT4_API int minigpt4_amd_end_chat_batch_sampled(struct MiniGPT4Context *ctx, const int32_t *slots, int n, const char **tokens, float temp, int32_t top_k, float top_p,
                                                     int32_t *ids_out);
MINIGPT4_API int minigpt4_amd_sampled_candidates(struct MiniGPT4Context *ctx, const int32_t *slots, int n, float temp, int32_t top_k, float top_p, int32_t *ids_out,
                                                 float *probs_out, int32_t *n_cand_out, int32_t *kept_out);
MINIGPT4_API int minigpt4_amd_conversation_seed(struct MiniGPT4Context *ctx, int slot, uint64_t seed, uint64_t draws);
MINIGPT4_API int minigpt4_amd_sampling_info(struct MiniGPT4Context *ctx, int slot, uint64_t out[6]);

/* ---- the extended rule: tail-free, typical and min-p filters, mirostat v2 with one mu per conversation ----------------------------------------------------------
 * The sampled step above honours temp, top_k and top_p.  The calls below honour every sampling parameter of minigpt4_end_chat except mirostat v1, and min_p (not in the
 * reference ABI; llama.cpp's later filter).  The generator, THE ROW and the CANDIDATES are the section's above, unchanged: n_c = min(top_k, participating ids) ids in that
 * order, values v_0 >= v_1 >= ..., top_k in 1 .. 64.  ARITHMETIC: fp32, each operation rounded on its own, nothing fused, sums sequential in list order.
 * THE LIVE LIST L is the ordered list of surviving candidate indices; it starts as all n_c candidates and always stays in value order.
 * softmax(L): a_j = expf(v_j - v_first(L)), A = the sequential sum, q_j = a_j / A; each filter recomputes it on the current L, as llama.cpp's chain does.
 * WITH mirostat == 0 the filters run in the order of the host chain, each keeping at least one candidate:
 *   1. tail-free, when tfs_z < 1 and |L| > 2: q = softmax(L), d1_i = q_i - q_{i+1}, d2_i = |d1_i - d1_{i+1}| for i < |L| - 2, s = sum d2; s > 1e-6f: d2_i = d2_i / s, else
 *      d2_i = 1.0f / (float)(|L| - 2); c += d2_i; at the first i >= 1 with c > tfs_z, L becomes its first i entries; none: L is unchanged.  (The host chain's tail_free.)
 *   2. typical, when typical_p < 1: q = softmax(L), H = sum -q_j * logf(q_j) (a term with q_j == 0 contributes 0), sh_j = fabsf(-logf(q_j) - H) (+inf where q_j == 0);
 *      L ordered by sh ascending, equal scores by list position; c += q in that order; kept through the first entry with c > typical_p, all if there is none.  The kept
 *      entries RETURN TO VALUE ORDER.  (A deliberate deviation: llama.cpp at the reference's revision leaves the list in typicality order, so its later softmax subtracts
 *      a value that need not be the maximum; the distribution is the same up to rounding.  Bit-equality with the host chain is not promised here, as it is not above.)
 *   3. top-p, when top_p < 1: step 1 of the rule above, on L.
 *   4. min-p, when min_p > 0: q = softmax(L); kept: the j with q_j >= min_p * q_first (one multiply) -- a prefix of L.
 *   5. temperature, softmax, draw: steps 2 - 4 of the rule above on L.  w_j = v_j / temp, b_j = expf(w_j - w_first), S the running sum over L in order,
 *      u = (float)(word >> 8) * 2^-24, t = u * S, the pick is the first entry with S_j > t, the last entry of L if there is none; p_j = b_j / S, 0 for a candidate not in L.
 *   NEUTRAL VALUES: with tfs_z = 1, typical_p = 1, min_p = 0 the chain performs exactly the operations of the rule above, in the same order: the pick, the kept count and
 *   every bit of every p_j are that rule's.
 * WITH mirostat == 2: llama.cpp's llama_sample_token_mirostat_v2 BEHIND top-k; tfs_z, typical_p, top_p and min_p are ignored, as the host chain ignores them there.
 *   w_j = v_j / temp, b_j = expf(w_j - w_0), Z = sum b_j, p_j = b_j / Z, s_j = -log2f(p_j); n = the first j with s_j > mu, n_c if there is none, 1 if that j is 0;
 *   S = the running sum of b_j for j < n; the draw is step 5's over those n; observed = -log2f(b_pick / S), e = observed - tau, mu' = mu - eta * e (the multiply and the
 *   subtract rounded separately).  Reported p_j = b_j / S for j < n, 0 behind.
 *   NOT THE REFERENCE'S BEHAVIOUR: the host chain's mirostat runs over the whole vocabulary, this one over at most 64 candidates.
 *   mu is a PER-CONVERSATION value: unset until the conversation's first mirostat decision, where it becomes 2 * tau.  Like (seed, draws) it belongs to the sampler:
 *   minigpt4_reset_chat, forks, shifts and snapshot loads leave it alone, minigpt4_amd_set_conversations unsets it, and it moves on every decision, whether or not the
 *   conversation then has room to advance.  The snapshot format stays version 1 and does not carry it.  (The host chain's mu is the context's: there, what a conversation
 *   receives depends on who shares its step.)
 * minigpt4_amd_end_chat_batch_sampled_ex: minigpt4_amd_end_chat_batch_sampled under this rule, step for step: one descriptor upload, one launch (kernel
 * k_sample_rows_ex: k_sample_rows' selection, then the chain), the picks handed to the pass on the device; mu' is read from the same pinned block as the picks, while the
 * pass runs.  draws += 1 per decision as above.
 * minigpt4_amd_sampled_candidates_ex: what the next such step would draw from: ids_out [n][64], probs_out [n][64], n_cand_out [n], kept_mask_out [n] (bit j: candidate j
 * is in L; under mirostat the low n bits); each may be NULL.  Nothing advances, no draw is counted, mu does not move.
 * minigpt4_amd_conversation_mirostat: a finite value sets the conversation's mu, NaN unsets it.
 * minigpt4_amd_mirostat_info: out = {set 0 / 1, mu (0 when unset), the last observed surprise, the tau it was measured against}.
 * Each returns 0, or 1 with "end_chat_batch_sampled_ex: ..." / "sampled_candidates_ex: ..." / "conversation_mirostat: ..." / "mirostat_info: ..." in
 * minigpt4_amd_last_error and nothing changed, before anything is decided: everything the plain calls refuse; tfs_z or typical_p outside (0, 1]; min_p outside [0, 1];
 * mirostat not 0 or 2 (1: "... mirostat v1 is not built"); mirostat_tau not finite or <= 0; mirostat_eta not finite or < 0; NaN in any of them; an infinite mu.
 * The buffers (a staging block of the extended descriptors and results) are allocated by the first _ex call and freed with the context and by
 * minigpt4_amd_set_conversations: a context that never calls these functions allocates nothing new and launches nothing new.  The existing calls launch k_sample_rows, one
 * instance of the source text both kernels share: its results are bit for bit what they were.  The counters of minigpt4_amd_sampling_info count the _ex calls too.
 * Not built: mirostat v1; mirostat over the whole vocabulary; mirostat inside draft verification (minigpt4_amd_verify_draft_sampled_ex below takes the filters only: mu at
 * row r would depend on row r - 1's pick); top_k = 0 or above 64; mu in snapshots; guided sampling on the device; a mode that redirects the reference's minigpt4_end_chat
 * here. */
MINIGPT4_API int minigpt4_amd_end_chat_batch_sampled_ex(struct MiniGPT4Context *ctx, const int32_t *slots, int n, const char **tokens, float temp, int32_t top_k, float top_p,
                                                        float tfs_z, float typical_p, float min_p, int mirostat, float mirostat_tau, float mirostat_eta, int32_t *ids_out);
MINIGPT4_API int minigpt4_amd_sampled_candidates_ex(struct MiniGPT4Context *ctx, const int32_t *slots, int n, float temp, int32_t top_k, float top_p, float tfs_z, float typical_p,
                                                    float min_p, int mirostat, float mirostat_tau, float mirostat_eta, int32_t *ids_out, float *probs_out, int32_t *n_cand_out,
                                                    uint64_t *kept_mask_out);
MINIGPT4_API int minigpt4_amd_conversation_mirostat(struct MiniGPT4Context *ctx, int slot, float mu);
MINIGPT4_API int minigpt4_amd_mirostat_info(struct MiniGPT4Context *ctx, int slot, float out[4]);

/* ---- speculation under sampling: drafts verified at temp > 0, lookup decoding with the reference's default sampler settings -----------------------------------
 * minigpt4_amd_verify_draft and minigpt4_amd_decode_lookup decide greedily.  Here the 1 + n rows of the same verify pass are SAMPLED, each with the draw plain decoding
 * would have used at its position.  A conversation's stream is counter-based (Philox, (seed, draws) above), so no rejection-sampling arithmetic is needed: a draft token
 * is kept exactly when the sample of the row before it equals it.  For a deterministic draft that accepts with probability P(draft token), the best any scheme achieves,
 * and the emitted tokens are the ones minigpt4_amd_end_chat_batch_sampled emits from the same state with the same (seed, draws) wherever the logits are the same: always in
 * parity mode; in fast mode a pass of another shape can round a logit differently, which can move a draw across a boundary.
 * THE RULE.  D(L, h, q, k) = the pick of the "sampled batched steps" rule above, unchanged: the raw row L after the conversation's logit bias and its penalties for the
 * token history h; only the ids allowed in constraint state q take part; top_k <= 64, then top_p, temperature, softmax; one draw with word 0 of Philox(seed, counter k).
 * Before the call the selected conversation has position p, raw logits L, history h, constraint state q and stream (seed, c).
 *   x0 = D(L, h, q, c).
 *   The pass evaluates rows t_0 = x0, t_{i + 1} = draft[i] at positions p, p + 1, ...; L_r = the logits of row r.
 *   h_r = h followed by t_0 .. t_r;  q_r = q walked over t_0 .. t_r (id 2 leaves the state, as minigpt4_amd_constraint_advance does).
 *   x_{r + 1} = D(L_r, h_r, q_r, c + 1 + r) for every evaluated row.
 *   m = the largest value with draft[i] == x_{i + 1} for all i < m.
 * AFTERWARDS ids_out[0 .. m] = t_0 .. t_m and *n_out = 1 + m; the conversation stands at p + 1 + m with the raw logits, greedy token and feed token of row m; its history
 * is h_m, its constraint state q_m, and draws = c + 1 + m: draws advance by exactly the number of tokens emitted.  The sample of row m is reported as *next_out and its draw
 * is NOT counted: the next decision of this conversation -- this call's x0, or minigpt4_amd_end_chat_batch_sampled -- recomputes the same token from the same row, state
 * and counter.  A caller drafts behind next_out; n_draft = 0 is one plain sampled step that also tells what comes next.  The call does not treat x0 == 2 specially.
 * minigpt4_amd_verify_draft_sampled: queued rows are evaluated first.  With the automatic shift on and no room for x0, x0's descriptor is built from the history before the
 * shift (as minigpt4_amd_end_chat_batch_sampled does) and the rows' from the shifted history followed by t_0 .. t_r.  The draft is cut to the room left, then at the first
 * token its constraint state does not allow (bit clear in the state's index row; id 2 is allowed exactly where the state accepts): a token that cannot be sampled cannot be
 * accepted.  A row where no id takes part picks "</s>" and is flagged stuck.  row_sampled_out (may be NULL; 1 + n_draft entries) = x_{r + 1} of every evaluated row, -1 for
 * a row that was not evaluated; row_logits_out (may be NULL; [1 + n_draft][n_vocab]) = the pass's raw rows, rows not evaluated are left alone.
 * ON THE DEVICE: x0 is one k_sample_rows launch on the conversation's row; the host waits for that 4-byte pick (the greedy call synchronises at the same point) because the
 * rows' histories and constraint states begin with it.  Then, behind one wait: the verify pass (captured per row count WITHOUT an epilogue -- the greedy passes keep
 * theirs), one k_sample_rows launch over the pass's R rows with R descriptors and draws c + 1 + r, and k_draft_sample_finish (one workgroup: m, row m into the
 * conversation's logits row with its first argmax from the same sweep, position, the result block).  Parity mode: one oracle-order single-row pass per row, each followed
 * by the decision on the conversation's own row, stopping at the first mismatch -- the sequence of minigpt4_amd_end_chat_batch_sampled there, bit for bit.
 * minigpt4_amd_decode_lookup_sampled: minigpt4_amd_decode_lookup's loop (the same drafter; history = corpus followed by the emitted tokens).  The first step runs with
 * n_draft = 0 to learn next_out; afterwards the draft continues the history behind next_out, cut at n_draft, before any id 2 and at the tokens still wanted.  With no match
 * the step is the n_draft = 0 pass again (one decision path, and it keeps announcing the next token).  Ends after max_tokens, after "</s>" has been emitted and
 * evaluated, or on a full context that cannot shift.  stats has minigpt4_amd_decode_lookup's meaning (passes + steps + accepted == *n_tokens).
 * minigpt4_amd_speculation_info: out = {sampled verify passes, rows evaluated, draft tokens sent, draft tokens accepted, sampling launches made by these calls, stuck picks,
 * draft tokens cut by a constraint, 0}.  The counters of minigpt4_amd_sampling_info do not count these calls; the conversation's draws does move.
 * Each returns 0, or 1 with "verify_draft_sampled: ..." / "decode_lookup_sampled: ..." / "speculation_info: ..." in minigpt4_amd_last_error and nothing changed, no draw
 * counted: no context, speculation off, n_draft outside the range, a NULL pointer (draft with n_draft > 0, ids_out, n_out, next_out; tokens_out, n_tokens, stats), an id
 * outside [0, n_vocab), no current logits, temp not finite or <= 0, top_k outside 1 .. min(64, n_vocab), top_p outside (0, 1], and "context full" when there is no room for
 * x0 and the automatic shift is off -- checked before anything is decided.  The graphs are dropped where the greedy ones are; the result block is allocated by the first
 * call: a context that never calls these functions allocates nothing new and launches nothing new.
 * Not built: several conversations' drafts in one pass; tree drafts; a draft model; remembering next_out per conversation, which would save the x0 launch of the next call
 * (every setter of bias, penalties, constraint, seed and logits would have to invalidate it); mirostat inside draft verification (mu at row r depends on row r - 1's
 * pick); guidance.
 * minigpt4_amd_verify_draft_sampled_ex / minigpt4_amd_decode_lookup_sampled_ex: the two calls with tfs_z, typical_p and min_p.  D(L, h, q, k) becomes the pick of the
 * extended rule above (mirostat == 0: tail-free, typical, top-p, min-p, temperature, softmax, draw); nothing else in THE RULE changes, so the emitted tokens are those of
 * minigpt4_amd_end_chat_batch_sampled_ex with the same parameters from the same (seed, draws) wherever the logits are the same.  On the device: k_sample_rows_ex and
 * k_draft_sample_finish_ex (k_draft_sample_finish's text over the extended result blocks) in the places of the plain kernels; with neutral values the results are the plain
 * calls'.  There are no mirostat arguments.  Refusals: the plain calls', under "verify_draft_sampled_ex: ..." / "decode_lookup_sampled_ex: ...", and tfs_z or typical_p
 * outside (0, 1], min_p outside [0, 1] (NaN included).  minigpt4_amd_speculation_info counts these calls too. */
MINIGPT4_API int minigpt4_amd_verify_draft_sampled(struct MiniGPT4Context *ctx, const int32_t *draft, int n_draft, float temp, int32_t top_k, float top_p, int32_t *ids_out,
                                                   int32_t *n_out, int32_t *next_out, int32_t *row_sampled_out, float *row_logits_out);
MINIGPT4_API int minigpt4_amd_decode_lookup_sampled(struct MiniGPT4Context *ctx, const int32_t *corpus, int n_corpus, int max_tokens, int ngram_max, int ngram_min, int n_draft,
                                                    float temp, int32_t top_k, float top_p, int32_t *tokens_out, int32_t *n_tokens, int32_t stats[4]);
MINIGPT4_API int minigpt4_amd_speculation_info(struct MiniGPT4Context *ctx, int64_t out[8]);
MINIGPT4_API int minigpt4_amd_verify_draft_sampled_ex(struct MiniGPT4Context *ctx, const int32_t *draft, int n_draft, float temp, int32_t top_k, float top_p, float tfs_z,
                                                      float typical_p, float min_p, int32_t *ids_out, int32_t *n_out, int32_t *next_out, int32_t *row_sampled_out,
                                                      float *row_logits_out);
MINIGPT4_API int minigpt4_amd_decode_lookup_sampled_ex(struct MiniGPT4Context *ctx, const int32_t *corpus, int n_corpus, int max_tokens, int ngram_max, int ngram_min, int n_draft,
                                                       float temp, int32_t top_k, float top_p, float tfs_z, float typical_p, float min_p, int32_t *tokens_out, int32_t *n_tokens,
                                                       int32_t stats[4]);

/* ---- speculation for SEVERAL conversations: the drafts of n conversations verified in one weight pass (greedy) --------------------------------------------------
 * minigpt4_amd_verify_draft puts 1 + n_draft rows of ONE conversation through a pass; the batched step (minigpt4_amd_end_chat_batch) puts ONE row of each of many through
 * it.  Here conversation slots[i] brings its greedy token g0_i and counts[i] draft tokens: a group of 1 + counts[i] rows at consecutive positions.  The groups are packed
 * into ONE pass of N = n + sum(counts) <= 64 rows -- the batched step's mat-vec launches at N rows (dot4 / row-interleaved MFMA up to 4 rows, the int8-MFMA set launches
 * from 5), an attention launch that is causal inside each group and reads nothing of another conversation, an epilogue with one decision per conversation -- and every
 * conversation keeps the guesses the pass's own logits confirm.  Needs minigpt4_amd_set_speculation(max_draft >= 1); the pass allocates N-row logits, a 128-word result
 * block and one captured pass per TOTAL row count at first use (the grouping is data in device memory: one graph serves every grouping), freed and dropped where the
 * single-conversation pass's are.  The plain step, the batched step and minigpt4_amd_verify_draft launch nothing new.
 * THE RULE, per conversation i, is minigpt4_amd_verify_draft's: g0_i = the first maximum of its RAW logits -- penalties, a logit bias and constraints do NOT enter it, nor
 * any row's decision; its tokens still enter the history --; g[r + 1] = the first argmax of its row r; m_i = the largest value with draft_i[j] == g[j + 1] for all j < m_i.
 * Afterwards ids_out[i][0 .. m_i] = g0_i, draft_i[0 .. m_i - 1], n_out[i] = 1 + m_i, the conversation stands at n_past = p_i + 1 + m_i with the logits, greedy token and
 * feed token of its row m_i.  Under greedy decoding every conversation's tokens are exactly those plain decoding emits.
 * minigpt4_amd_verify_draft_batch: slots[n] distinct; drafts = the drafts concatenated in list order (as minigpt4_amd_score_batch takes its tokens), counts[n] each in
 * [0, max_draft]; ids_out [n][8]; n_out [n]; row_greedy_out (may be NULL) [n][8] = g[1 ...] of every evaluated row, -1 behind them.  Queued prompt rows of every listed
 * conversation are evaluated first (as minigpt4_amd_end_chat_batch does).  A draft longer than the room left is cut to n_ctx - n_past - 1 rows; a conversation with no
 * room for g0 follows the batched step: the automatic shift makes room, else n_out[i] = 0 and the conversation is left out of the pass, untouched.  One wait per call.
 * The sampler's generator, the mirostat state and the prefix cache are untouched.  Every count 0 (or cut to 0): the ordinary batched step -- its own graph, its own
 * epilogue -- so a call without drafts costs what minigpt4_amd_eval_batch costs.  Parity mode: minigpt4_amd_verify_draft's one-row oracle-order loop per conversation,
 * bit-identical to plain greedy decoding, no speed-up.  No key-split attention in the pass.
 * Refused (1, "verify_draft_batch: ...", nothing changed -- except that "a conversation has no current logits" can also come AFTER the queued prompt rows of the
 * conversations listed before it were evaluated, as in minigpt4_amd_end_chat_batch: their rows then stand evaluated, no token is emitted): no context, speculation off, slots NULL / n < 1 / n above the conversations, a duplicate or out-of-range slot,
 * counts / ids_out / n_out NULL, a count outside [0, max_draft], drafts NULL with a count > 0, an id outside [0, n_vocab), a conversation without current logits, more
 * than 64 rows in total (or more than the context's activation rows, max(n_batch, 32, conversations)).
 * minigpt4_amd_decode_lookup_batch: minigpt4_amd_decode_lookup's loop over n conversations.  Each has its own drafter -- history = its corpus (corpus: the corpora
 * concatenated, corpus_counts[i] tokens each, 0 allowed) followed by what IT has emitted --, its own max_tokens budget and its own end (</s> emitted and evaluated, or a
 * full context that cannot shift); every iteration is one minigpt4_amd_verify_draft_batch over the conversations still running (drafts are shortened, in list order,
 * where the pass's 64 rows would not hold them).  tokens_out [n][max_tokens], n_tokens [n], stats [n][4] = {passes in which the conversation sent a draft, passes in
 * which it sent none, draft tokens sent, draft tokens accepted} (passes + steps + accepted == n_tokens[i]).  Refusals: minigpt4_amd_decode_lookup's and the slot
 * list's, under "decode_lookup_batch: ...".
 * minigpt4_amd_speculation_batch_info: out = {passes, rows evaluated, groups, draft tokens sent, draft tokens accepted, calls without a draft that took the plain
 * batched step, draft tokens cut for room, 0} since the context was loaded; parity mode's one-row loops are not passes of this kind and count nothing but the cut.  minigpt4_amd_speculation_info does not count these calls.
 * BREAK-EVEN: a pass of N rows for n conversations pays when the draft tokens kept per conversation per pass exceed pass_ms(N) / step_ms(n) - 1, step_ms(n) = the
 * batched step at n rows.  WHICH n_draft: tools/lookup_batch_decode.py prints pass_ms, step_ms and that break-even per (n, rows per conversation).  Recorded
 * (profiles/r19_lookup_batch.log, 13B Q5_K_M, about 150 cached keys, medians of 5): rows per conversation 2 / 4 / 8 need 0.18 / 0.66 / 0.78 kept draft tokens per
 * conversation per pass at n = 2, 0.43 / 0.53 / 0.76 at n = 4, 0.10 / 0.25 / 0.80 at n = 8 -- the steps in pass_ms lie at 5 rows (the int8-MFMA set launches) and
 * above 32.  Synthetic files: nothing is measured about how many draft tokens real text keeps. */
MINIGPT4_API int minigpt4_amd_verify_draft_batch(struct MiniGPT4Context *ctx, const int32_t *slots, int n, const int32_t *drafts, const int32_t *counts, int32_t *ids_out,
                                                 int32_t *n_out, int32_t *row_greedy_out);
MINIGPT4_API int minigpt4_amd_decode_lookup_batch(struct MiniGPT4Context *ctx, const int32_t *slots, int n, const int32_t *corpus, const int32_t *corpus_counts, int max_tokens,
                                                  int ngram_max, int ngram_min, int n_draft, int32_t *tokens_out, int32_t *n_tokens, int32_t *stats);
MINIGPT4_API int minigpt4_amd_speculation_batch_info(struct MiniGPT4Context *ctx, int64_t out[8]);

/* ---- snapshots: save and restore a conversation --------------------------------------------------------------------------------------------------------
 * A conversation leaves its slot, its context or its process as one blob (llama.cpp's llama_copy_state_data / session files / slot save and restore) and comes back bit
 * for bit: a restored conversation continues with the logits and tokens of the uninterrupted one.  The cache rows travel through k_kv_pack / k_kv_unpack -- rows
 * [r0, r0 + n) of every layer, keys and values, to / from one contiguous block per launch, with the block's checksum (the wrapping 64-bit sum of its 32-bit words)
 * computed in the same sweep.
 * FORMAT, version 1.  Little-endian; a blob may start at any address.
 *   header, 64 bytes:  0 magic "MG4S" | 4 u32 version = 1 | 8 u64 total bytes | 16 u32 n_layer | 20 u32 n_embd | 24 u32 n_head | 28 u32 n_vocab | 32 u64 LLM arena hash
 *     (what minigpt4_amd_arena_plan reports) | 40 u32 n_rows | 44 u32 block_rows | 48 u32 flags (bit 0: has a logits row, bit 1: saved in parity mode) | 52 i32 greedy
 *     token | 56 i32 feed token | 60 u32 n_bias
 *   sections, back to back from byte 64:
 *     token history   n_rows x i32, the token id of every cache row, -1 for an embedding row
 *     logits row      n_vocab x f32, present only with flag bit 0
 *     penalties       i32 repeat_last_n, f32 repeat_penalty, f32 alpha_presence, f32 alpha_frequency, i32 penalize_nl
 *     logit bias      n_bias x (i32 id, f32 bias), n_bias <= 256
 *     zero padding to a multiple of 8, then the block table: one u64 checksum per block, ceil(n_rows / block_rows) of them
 *     zero padding to a multiple of 16, then the KV blocks, one per block_rows rows, the last one short: [tensor K, V][layer][row][n_embd] fp16, i.e.
 *     4 * n_layer * n_embd bytes per row
 *   block_rows = max(1, block_bytes / bytes per row); block_bytes is 32 MiB unless MINIGPT4_STATE_BLOCK_BYTES (read by minigpt4_model_load) says otherwise.  A loader
 *   takes block_rows from the blob, whatever its own setting.
 * NOT in a snapshot: the sampler's generator and the mirostat state (they belong to the context); the constraint handle and state (handles are per context: a load
 *   keeps the slot's handle and returns its state to the start, like minigpt4_reset_chat); queued rows (a save evaluates them first); the prefix store.
 * minigpt4_amd_state_size: the bytes a save of `slot` would take now, queued rows counted; 0 for a slot out of range.
 * minigpt4_amd_state_save: *written (may be NULL) = the size.  cap too small (or buf NULL): 1, *written = the size needed, nothing written, nothing evaluated.
 * minigpt4_amd_state_load: the header and every host section are checked BEFORE anything on the device or in the conversation changes: magic, version, total bytes ==
 *   n, section sizes, the model fingerprint (n_layer, n_embd, n_head, n_vocab, arena hash), n_rows <= n_ctx, every history id in [-1, n_vocab), the penalty and bias
 *   values the setters would accept.  Then whatever the slot held, queued rows included, is dropped, the blocks are uploaded and unpacked, and position, logits row,
 *   greedy and feed token, history, penalties and bias are installed: minigpt4_end_chat, the batched step, scoring, fork, shift and minigpt4_amd_verify_draft continue
 *   from there.  The target slot may be any slot of any context loaded from the same language-model file (n_ctx may differ as long as the rows fit).
 *   A block whose checksum differs from the table ends the call with 1 and "state_load: block c checksum"; the conversation is then left as minigpt4_reset_chat
 *   leaves it.  This is the ONE failure that is not "nothing changed": its rows were already overwritten.
 * minigpt4_amd_state_save_file / _load_file: the same through a file; save writes path + ".tmp" and renames it.
 * minigpt4_amd_state_peek: needs no context and no GPU.  Runs every check that needs no context and reports out = {version, total bytes, n_layer, n_embd, n_head,
 *   n_vocab, arena hash, n_rows, block_rows, flags, greedy token, feed token}.
 * minigpt4_amd_state_info: out = {saves, loads, rows saved, rows loaded, k_kv_pack launches, k_kv_unpack launches, checksum failures, bytes of staging held}.  The
 *   staging -- two device and two pinned blocks, the checksum words, a copy stream -- is allocated by the first save or load, survives
 *   minigpt4_amd_set_conversations and is freed with the context; a context that never calls these entry points allocates and launches nothing new.
 * Each call returns 0, or 1 with "<short name>: ..." in minigpt4_amd_last_error.
 * Not built: incremental snapshots (the kernels take a row range, so only new rows could be appended later), compression or a narrower cache type, constraint state,
 * snapshots across different weight files. */
MINIGPT4_API size_t minigpt4_amd_state_size(struct MiniGPT4Context *ctx, int slot);
MINIGPT4_API int minigpt4_amd_state_save(struct MiniGPT4Context *ctx, int slot, void *buf, size_t cap, size_t *written);
MINIGPT4_API int minigpt4_amd_state_load(struct MiniGPT4Context *ctx, int slot, const void *buf, size_t n);
MINIGPT4_API int minigpt4_amd_state_save_file(struct MiniGPT4Context *ctx, int slot, const char *path);
MINIGPT4_API int minigpt4_amd_state_load_file(struct MiniGPT4Context *ctx, int slot, const char *path);
MINIGPT4_API int minigpt4_amd_state_peek(const void *buf, size_t n, int64_t out[12]);
MINIGPT4_API int minigpt4_amd_state_info(struct MiniGPT4Context *ctx, int64_t out[8]);

/* ---- weight arenas (load-time broadcast rank0 -> others over RCCL) ---------------------------- */
/* which: 0 = LLM arena, 1 = vision arena.  Returns the device pointer and size in bytes. */
MINIGPT4_API int minigpt4_amd_weight_arena(struct MiniGPT4Context *ctx, int which, void **device_ptr, size_t *bytes);
/* Multi-GPU load (replicas; the only exchange is the load-time broadcast of the two weight arenas from rank 0).  Rank 0 loads normally; the other ranks
 * set MINIGPT4_LOAD=recv before minigpt4_model_load: headers are parsed, both arenas are laid out and allocated exactly as rank 0's (compare minigpt4_amd_arena_plan), no
 * tensor data is read, uploaded or repacked; after the arenas have been received (minigpt4_amd_weight_arena gives the device ranges) minigpt4_amd_weights_received builds
 * what is derived from them on the device.  minigpt4_amd_plan_arenas computes the same layout from the files alone, without a GPU. */
/* The same exchange INSIDE minigpt4_model_load, for clients without Python / torch (csrc/dist.cpp): with MINIGPT4_WORLD_SIZE = N, MINIGPT4_RANK = r and
 * MINIGPT4_NCCL_ID_FILE = <a path every rank of the job can read, unique to the job> in the environment, rank 0 loads the files, writes the ncclUniqueId to that file and
 * broadcasts both arenas (librccl.so by dlopen, <= 1 GiB pieces); ranks 1..N-1 load headers only, wait for the id (MINIGPT4_DIST_TIMEOUT_S, default 120), receive, finish
 * the load; layout hashes before and arena checksums after must agree.  Any failure fails the load (NULL; text in minigpt4_amd_last_error) -- no fallback to the files.
 * One process per GPU: MINIGPT4_DEVICE (or LOCAL_RANK) selects it.  minigpt4_amd_dist_info: what this context's load did (bcast_ms = 0 for an ordinary load). */
MINIGPT4_API int minigpt4_amd_dist_info(struct MiniGPT4Context *ctx, int *world, int *rank, float *bcast_ms);
MINIGPT4_API int minigpt4_amd_plan_arenas(const char *vision_path, const char *llm_path, size_t *llm_bytes, size_t *vision_bytes, uint64_t *llm_hash, uint64_t *vision_hash);
MINIGPT4_API int minigpt4_amd_arena_plan(struct MiniGPT4Context *ctx, size_t *llm_bytes, size_t *vision_bytes, uint64_t *llm_hash, uint64_t *vision_hash);
MINIGPT4_API int minigpt4_amd_load_mode(struct MiniGPT4Context *ctx);              /* 0 full, 1 waiting for the arenas */
MINIGPT4_API int minigpt4_amd_weights_received(struct MiniGPT4Context *ctx);
MINIGPT4_API int minigpt4_amd_arena_checksum(struct MiniGPT4Context *ctx, int which, uint64_t *sum);   /* 64-bit sum of the arena's 32-bit words (device reduction) */

/* Image file decoding from memory (the host half of minigpt4_image_load_from_file; the request server takes images as bytes): PNG / JPEG / BMP / binary PNM bytes -> U8 HWC RGB
 * with cv::imread(IMREAD_COLOR)+BGR2RGB semantics.  The library allocates image->data; release with minigpt4_free_image.  0 or 5 (OpenImage). */
MINIGPT4_API int minigpt4_amd_decode_image(const void *bytes, size_t n, OUT struct MiniGPT4Image *image);

#ifdef __cplusplus
}
#endif
