// MI355X MiniGPT-4 engine: owns HBM arenas (weights repacked into planes, fp16 KV cache, activation buffers), the HIP stream
// and the decode hipGraph.  Mirrors the call surface of the reference's `class MiniGPT4` (minigpt4.cpp:1740-2522):
// init / encode_image / add_tokens / add_strings / add_embedding / sample_token / id_to_token / reset.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "common.hpp"
#include "formats.hpp"
#include "kernels.hpp"
#include "owned.hpp"
#include "pick_stage.hpp"
#include "sampler.hpp"
#include "state.hpp"

namespace mg4 {

struct DeviceArena {
    uint8_t *base = nullptr;
    size_t cap = 0, used = 0;
    bool virt = false;                       // planning only (Engine::plan_arenas): no device memory, `base` is a fake non-null address that is never dereferenced
    uint64_t layout_hash = 1469598103934665603ull;   // FNV-1a over the (offset, bytes) sequence of take(): two loads with the same hash laid the arena out identically
    void alloc(size_t bytes);
    void release();
    uint8_t *take(size_t bytes, size_t align = 256);
    void abandon() { base = nullptr; cap = used = 0; }   // leak on purpose: hipFree synchronises with a stream that will never drain (Engine::stream_hung_)
    ~DeviceArena() { release(); }
};


class Engine {
public:
    Engine() = default;
    ~Engine();
    int init(const std::string &vision_path, const std::string &llm_path, int seed, int n_ctx, int n_batch);
    // ---- multi-GPU load: rank 0 loads the files (LOAD_FULL) and broadcasts its two weight arenas; the other ranks run LOAD_RECV:
    // parse the HEADERS only, lay the arenas out identically (same take() sequence -> same layout hash), allocate them, skip every file read / upload
    // / repack, receive the bytes, then call weights_received() for what is derived on the device (prefill planes, the replicated query tokens).
    // LOAD_PLAN does the layout without any device (CPU tests).
    enum LoadMode { LOAD_FULL = 0, LOAD_RECV = 1, LOAD_PLAN = 2 };
    int weights_received();
    struct ArenaPlan { size_t llm_bytes = 0, vision_bytes = 0; uint64_t llm_hash = 0, vision_hash = 0; };
    static int plan_arenas(const std::string &vision_path, const std::string &llm_path, ArenaPlan &out);   // host only
    ArenaPlan arena_plan() const { ArenaPlan p; p.llm_bytes = llm_arena_.used; p.vision_bytes = vis_arena_.used; p.llm_hash = llm_arena_.layout_hash; p.vision_hash = vis_arena_.layout_hash; return p; }
    LoadMode load_mode() const { return load_mode_; }
    // native broadcast (dist.hpp): what this context's load did -- world size, rank, milliseconds of the exchange (0 when the load was an ordinary
    // one)
    int dist_world() const { return dist_world_; }
    int dist_rank() const { return dist_rank_; }
    float dist_bcast_ms() const { return dist_bcast_ms_; }

    // ---- image path (reference encode_image, minigpt4.cpp:2094-2363)
    int encode_image(const float *chw, float *out);   // out: [32][proj_out()]
    int encode_images(const float *const *chw, int B, float *const *out);   // B <= VISION_BATCH_MAX images in one pass over the vision weights
    static constexpr int VISION_BATCH_MAX = 8;
    int proj_out() const { return v_out_; }
    int n_query() const { return v_nq_; }

    // ---- language path
    int add_tokens(const std::vector<int> &tokens, bool flush_now = false);   // queued; evaluated in chunks of n_batch (minigpt4.cpp:2365-2382)
    int flush();                                      // evaluate everything queued by add_tokens / add_embedding
    int add_string(const std::string &s);             // BOS + tokenize (minigpt4.cpp:2384-2397)
    int add_embedding(const float *data, int n_rows); // llama_eval_embd (minigpt4.cpp:2399-2422)
    int sample_token(const SampleParams &p);          // minigpt4.cpp:2425-2483
    const char *id_to_token(int id) const;            // minigpt4.cpp:2485-2497 (borrowed pointer)
    // minigpt4.cpp:2499-2502 (the selected conversation)
    void reset() { Conversation &c = conv_[(size_t)cur_]; c.n_committed = 0; c.hist.clear(); c.drop_queue(); c.has_logits = false; con_state_[cur_] = con_handle_[cur_] ? CONSTRAINT_START : 0; }
    void sync();
    hipStream_t stream() const { return stream_; }
    // ---- context shift (llama.cpp's answer to a full context), selected conversation: pending rows are evaluated first, then rows
    // [n_keep, n_keep + n_discard) are dropped and the rows above slide down in place, their keys re-rotated by -n_discard positions
    // (launch_kv_shift).  The last logits stay valid; captured graphs too (positions are read from d_npast_).  0, or 1 with last_error set and the
    // conversation untouched (n_keep < 0, n_discard < 0, n_keep + n_discard > n_past).
    int shift_context(int n_keep, int n_discard);
    // automatic policy (per context, off = -1 by default): an add that would overflow first shifts by max(need, (n_past - n_keep) / 2) rows; a full
    // conversation in decode_batch is shifted and advanced.  An add longer than n_ctx - n_keep still fails.
    void set_context_shift(int n_keep) { shift_keep_ = n_keep < 0 ? -1 : n_keep; }

    int n_vocab() const { return (int)llm_.n_vocab; }
    int n_embd() const { return (int)llm_.n_embd; }
    int n_past() const { return conv_[(size_t)cur_].n_past; }
    int n_ctx() const { return n_ctx_; }
    const LaunchTuning &launch_tuning() const { return tune_; }
    const float *logits_host();                       // syncs, copies the last logits to pinned memory
    const Tokenizer &tokenizer() const { return tok_; }
    size_t weight_bytes_per_token() const { return wbytes_token_; }
    size_t llm_arena_bytes() const { return llm_arena_.used; }
    size_t vision_arena_bytes() const { return vis_arena_.used; }
    uint8_t *llm_arena_ptr() { return llm_arena_.base; }
    uint8_t *vision_arena_ptr() { return vis_arena_.base; }

    // ---- several conversations per replica.  The reference holds ONE conversation per context (minigpt4.cpp:2513-2521); here a
    // context owns n >= 1 of them -- each with its own KV cache region, position and pending queue, sharing the weights -- so that a decode step of B
    // conversations streams the weights once instead of B times.  All reference entry points act on the selected conversation (0 by default).
    int set_conversations(int n);                      // (re)allocates the KV caches; every conversation is reset.  1 <= n <= MAX_CONVERSATIONS
    int select_conversation(int slot);
    int n_conversations() const { return (int)conv_.size(); }
    int current_conversation() const { return cur_; }
    // one decode step for `n` distinct conversations: sample each (like sample_token), evaluate the n sampled tokens in ONE weight pass. ids_out[i] =
    // the token sampled for slots[i]; a conversation whose context is full is sampled but not advanced (the reference discards the error too).
    // forced != null: the step evaluates forced[i] for slots[i] instead of the token it sampled (teacher forcing: tests / bench parity legs compare every step's logits with
    // an oracle conversation that is fed the same ids); ids_out still reports what the conversation's own logits chose
    // top (decode_batch_top below): also report the distribution every id was drawn from
    struct TopOut { int top_n = 0; int *top_ids = nullptr; float *top_lp = nullptr, *logprob = nullptr; int *rank = nullptr; };
    int decode_batch(const int *slots, int n, const SampleParams &p, int *ids_out, const int *forced = nullptr, const TopOut *top = nullptr);
    // the queued prompt rows of `n` distinct conversations, packed into chunks of <= n_batch rows, one pass over the weights per chunk.  Afterwards each is
    // where its own flush() leaves it (n_committed == n_past, queue empty, last-row logits / greedy id / feed token in its slot); one with nothing queued is
    // skipped.  0, or 1 (bad slot list, failed pass: then every listed conversation drops its queue, n_past = n_committed, like a failed flush).  Parity
    // mode and the parity trace: one flush() per conversation in slot order.
    int prefill_batch(const int *slots, int n);
    // Which launches the LAST BUILT batched step (forward_batch: eager, or the capture of a graph) took, per kind -- so that a test / the bench can assert that the
    // operating point it means to check (k_matvec_ri, k_matvec_ri_mix, the K-split w2 launch) is the one that ran, instead of a fallback with the same results
    struct BatchPath { int rows = 0, ri = 0, ri_mix = 0, ri_ksplit = 0, dot4 = 0, dot4_mix = 0, mul_mat = 0, sets = 0, ri_plain = 0; };
    const BatchPath &batch_path() const { return batch_path_; }
    static constexpr int MAX_CONVERSATIONS = 64;

    // ---- reuse of cached rows.  The K / V rows of a causal model depend only on the rows before them, so a prefix evaluated once can be COPIED into another
    // conversation instead of being evaluated again (launch_kv_copy: one launch for every layer, keys and values, every destination).  Exact in parity mode; in
    // fast mode the rows after the prefix run at a different N (the K split of the prompt mat-muls depends on N): inside the bound the batched prefill is tested to.
    // fork: conversation src -> n_dst other conversations.  n_rows = -1: the whole state -- the source's queue is evaluated first, then its n_committed rows, its
    // logits row, greedy id and feed token are copied: every destination can be sampled at once and equals the source.  0 <= n_rows <= n_past(src): that prefix
    // only (the queue is evaluated first when it reaches into it); the destinations end at n_past = n_committed = n_rows with no current logits, like after
    // reset(): the caller adds rows before sampling.  A destination's queue is dropped, its captured graph kept (positions are read from d_npast_).  0, or 1 with
    // last_error "fork_conversation: ..." and everything untouched (src / a destination out of range, duplicates, a destination equal to src, n_dst < 1,
    // n_rows < -1 or > n_past(src)).
    int fork(int src, const int *dst, int n_dst, int n_rows);
    // prefix store (off by default): ONE stored prefix -- the token ids and K / V rows [layer][max_rows][E] of the leading token run of a pass that started at
    // position 0.  Lookup (flush / prefill_batch, a conversation at n_committed == 0): m = the common prefix of its queue's leading token run with the stored ids,
    // capped at queue length - 1 (one row is always evaluated, so that logits exist); m >= PREFIX_MIN_ROWS: the m rows are copied from the store and the pass starts
    // at row m (a batched call serves all its hits with one launch).  Capture (after a successful pass from position 0, at most one per call, the first qualifying
    // conversation in slot-list order): a leading run of >= PREFIX_MIN_ROWS token rows that the store did not cover (m < min(run, max_rows)) overwrites the store
    // with its first min(run, max_rows) rows.  So a constant system prompt + "Human: <Img>" (the run ends at the image rows) is captured once and never rewritten,
    // while a text-only chat, whose run is its whole queue and is therefore never covered, re-captures its own run every time (one cheap copy).
    // set_prefix_cache: 0 = off, the store is freed; > 0 (clamped to n_ctx): (re)allocated when the size changes, emptied, counters zeroed.  set_conversations
    // and a set_parity that changes the mode empty it (parity-mode rows must come from parity-mode passes).
    static constexpr int PREFIX_MIN_ROWS = 8;          // policy: a bare BOS / a few common words are not worth a launch
    int set_prefix_cache(int max_rows);
    // hit_launches: k_kv_copy launches made by lookups (a batched call with 4 hits adds 1); rows_last: rows the last pass that consulted the store took from it
    struct PrefixInfo { int max_rows = 0, stored_rows = 0, hits = 0, rows_reused_total = 0, captures = 0, rows_last = 0, hit_launches = 0; };
    PrefixInfo prefix_info() const { PrefixInfo p = pfx_; p.max_rows = pfx_max_; p.stored_rows = (int)pfx_ids_.size(); return p; }

    // ---- scoring: the log-probabilities of GIVEN tokens (llama.cpp's logits_all / perplexity), from the prompt pass that evaluates them.  Entry i describes the
    // distribution tokens[i] is drawn from: for i >= 1 the logits of row i - 1 of this call, for i == 0 the conversation's logits from before the call (none --
    // nothing evaluated yet, after reset(), after a partial fork: logprob 0, greedy -1, greedy_logprob 0, a zero logits row).  logprob[i] = log softmax(row)[tokens[i]],
    // greedy[i] = the row's first argmax, greedy_logprob[i] = its log-probability, logits_out[i] = the row.  The pass is the one add_tokens + flush runs -- same chunks,
    // same launches, the last row's logits / greedy id / feed token from the same one-row output launch -- with the scored rows' output mat-mul (tiles of SCORE_ROWS
    // rows into a buffer of the feature's own) and k_logprob_rows next to it, so the conversation ends bit-identical and can be sampled and continued.  The prefix
    // store is neither consulted nor written.  0, or 1 with last_error "score_tokens: ..." and nothing of `tokens` added (null tokens / logprob, n < 1, an id outside
    // [0, n_vocab) -- checked on the host: a target indexes a logits row on the device --, rows that do not fit n_ctx under add_tokens' rule).
    static constexpr int SCORE_ROWS = 64;
    int score_tokens(const int *tokens, int n, float *logprob, int *greedy, float *greedy_logprob, float *logits_out);
    // the same for n_slots distinct conversations, tokens / counts / outputs concatenated in slot-list order: queued rows first (prefill_batch), then every
    // conversation's tokens packed into as few passes as prefill_batch takes; each conversation ends bit-identical to prefill_batch of the same tokens.  Parity mode:
    // one score_tokens per conversation.  1 with last_error "score_batch: ..." and every conversation untouched on a bad slot list, a count < 1, a bad id, an overflow
    // (all checked before anything runs).  A pass or an automatic shift that fails on the device afterwards also returns 1 with that prefix; conversations the call had
    // already evaluated or shifted by then keep that state, as after a failed prefill_batch.
    int score_batch(const int *slots, int n_slots, const int *tokens, const int *counts, float *logprob, int *greedy, float *greedy_logprob);

    // ---- top-N alternatives (k_topn_rows): the first top_n (1 .. TOPN_MAX, <= n_vocab) tokens of a distribution in the order "logit descending, equal logits by
    // ascending id", their log-probabilities (log-softmax of the RAW logits, whatever the sampling parameters), and the rank of a given token in that order.  Every
    // check comes before anything runs; a refusal returns 1 with last_error "<name>: ..." and changes nothing.
    // what each listed DISTINCT conversation would say next: queued rows first (prefill_batch(slots, n)), then one launch over the listed rows of logits_, one copy
    // back, one synchronise.  targets (may be null; -1 = none): logprob / rank (may be null) describe targets[i].  A conversation without current logits: ids -1,
    // log-probabilities 0, rank -1.  Position, logits, greedy / feed token, the sampler's generator and mirostat state are untouched.
    int top_logprobs(const int *slots, int n, int top_n, const int *targets, int *top_ids, float *top_lp, float *logprob, int *rank);
    // decode_batch that also reports, per listed conversation (one sampled but not advanced included), the sampled id's log-probability and rank and the top_n
    // alternatives of the distribution it was drawn from: the kernel runs on the n logits_ rows after the sampling and before the weight pass (one in-order stream),
    // its copy back is queued before the step and awaited after the step is launched.  Conversations, ids and sampler draws are decode_batch's.
    int decode_batch_top(const int *slots, int n, const SampleParams &p, int *ids_out, const TopOut &top);
    // score_tokens with the rank of every given token and the alternatives of the distribution it is drawn from (entry indexing as score_tokens; entry 0 without
    // logits: logprob 0, rank -1, ids -1, log-probabilities 0).  The same passes and the same k_logprob_rows launches as score_tokens -- logprob and the conversation
    // afterwards are bit for bit its -- with k_topn_rows behind k_logprob_rows on every tile.
    int score_tokens_top(const int *tokens, int n, int top_n, float *logprob, int *rank, int *top_ids, float *top_lp);

    // ---- speculation, greedy: one conversation puts several of its OWN rows through one weight pass.  verify_draft evaluates the rows g0, draft[0 .. n) (g0 = the
    // selected conversation's greedy token) at consecutive positions in a verify pass of forward_batch (causal among the rows: launch_attn_llm_draft) and keeps the
    // 1 + m rows whose tokens the pass's own logits chose: ids_out = g0, draft[0 .. m), *n_out = 1 + m, n_past = n_committed = p + 1 + m, logits / greedy / feed token
    // those of row m.  Cache rows above n_past hold the rejected rows' keys and values: dead (fork copies n_committed rows, the next evaluation overwrites them).
    // row_greedy (may be null, 1 + n_draft entries): the first argmax of every evaluated row, -1 for rows not evaluated (cut for room; parity mode: behind the first
    // mismatch).  n_sent (may be null): draft rows evaluated.  Parity mode: one single-row oracle-order pass per row, stopping at the first mismatch.
    // set_speculation allocates (1 + max_draft) logits rows, the result block and its pinned mirror, one graph slot per row count; 0 frees them.  It never builds the
    // row-interleaved MFMA image: a context that has it (set_conversations(n > 1)) uses it at 3 and 4 rows.  The setting survives set_parity / set_conversations; the
    // captured passes are dropped there with the batched ones.  1 + last_error "set_speculation: ..." / "verify_draft: ..." / "decode_lookup: ..." on a refusal.
    static constexpr int DRAFT_MAX = DRAFT_ROWS - 1;
    int set_speculation(int max_draft);
    int verify_draft(const int *draft, int n_draft, int *ids_out, int *n_out, int *row_greedy, int *n_sent = nullptr);
    // the greedy generation loop over an n-gram drafter (draft.hpp): history = corpus + what this call emitted; a pass with a draft where the history's suffix occurs
    // earlier, the ordinary decode step (sample_token at temp 0 + add_tokens, its own graph, key-split attention included) where it does not.
    // stats = {verify passes, plain steps, draft tokens sent, draft tokens accepted}
    int decode_lookup(const int *corpus, int n_corpus, int max_tokens, int ngram_max, int ngram_min, int n_draft, int *tokens_out, int *n_tokens, int *stats);
    // ---- speculation under sampling (temp > 0; minigpt4_amd.h: the rule; draft_host.hpp: the host staging).  The conversation's stream is counter-based, so every row of the
    // pass is sampled with the draw plain decoding would use at its position and a draft token is kept exactly when the sample equals it: the emitted tokens are those of
    // decode_batch_sampled from the same (seed, draws) wherever the logits are the same.  verify_draft_sampled: x0 = the decision of the existing launch_sample_rows on the
    // conversation's logits_ row (descriptor from the history before an automatic shift); the host waits for that pick -- the greedy call synchronises at the same point --
    // because the rows' histories and constraint states start with it; draft_stage builds the R descriptors (tables over the shifted history + t_0 .. t_r, states q_r, the
    // constraint's cut); then, behind ONE wait: the slab's copy, the verify pass WITHOUT an epilogue (forward_batch(R, verify, epilogue = false), one captured graph per row
    // count in spec_sgraph_ -- the greedy graphs in spec_graph_ end in launch_draft_finish and stay as they are), and behind it, launched eagerly, launch_sample_rows over
    // spec_logits_ with draws c + 1 + r and launch_draft_sample_finish, the result block's copy.  The epilogue stays outside the graph because its descriptor upload has a
    // length of its own every call and its buffers (the smp_* staging, freed by set_conversations) have another lifetime than the pass's.  Afterwards: n_past = p + 1 + m,
    // history + t_0 .. t_m, constraint state q_m, draws = c + 1 + m (the sample of row m is reported as *next_out, its draw not counted: the next decision recomputes it).
    // row_sampled (may be null, 1 + n_draft entries): x_{r + 1} of every evaluated row, -1 behind them; row_logits (may be null): the pass's raw rows [1 + n_draft][n_vocab],
    // evaluated rows only.  Parity mode: one oracle-order single-row pass per row, each followed by the decision on the conversation's own row, stopping at the first
    // mismatch -- decode_batch_sampled's own sequence.  The graphs are dropped with the greedy ones; the result block is allocated by the first call.  The counters of
    // sampling_info do not count these launches; speculation_info does.  1 + last_error "<name>: ..." and nothing changed on a refusal.
    int verify_draft_sampled(const int *draft, int n_draft, float temp, int top_k, float top_p, int *ids_out, int *n_out, int *next_out, int *row_sampled, float *row_logits,
                             const char *name = "verify_draft_sampled", int *n_sent = nullptr);
    // decode_lookup's loop under sampling: the drafter drafts behind next_out (the first step runs with n_draft = 0 to learn it); no match: the n_draft = 0 pass again -- a
    // plain sampled step that also tells what comes next, so the loop needs no second decision path
    int decode_lookup_sampled(const int *corpus, int n_corpus, int max_tokens, int ngram_max, int ngram_min, int n_draft, float temp, int top_k, float top_p, int *tokens_out,
                              int *n_tokens, int *stats);
    // the two calls with D(L, h, q, k) = the extended rule's chain (tfs_z, typical_p, min_p of cp; mirostat is not available here: mu at row r would depend on row
    // r - 1's pick): the same bodies (verify_draft_sampled_t / decode_lookup_sampled_t), the extended staging block, k_sample_rows_ex and k_draft_sample_finish_ex
    int verify_draft_sampled_ex(const int *draft, int n_draft, float temp, int top_k, float top_p, const ChainParams &cp, int *ids_out, int *n_out, int *next_out, int *row_sampled,
                                float *row_logits);
    int decode_lookup_sampled_ex(const int *corpus, int n_corpus, int max_tokens, int ngram_max, int ngram_min, int n_draft, float temp, int top_k, float top_p, const ChainParams &cp,
                                 int *tokens_out, int *n_tokens, int *stats);
    // {sampled verify passes, rows evaluated, draft tokens sent, draft tokens accepted, sampling launches made by these calls, stuck picks, draft tokens cut by a constraint, 0}
    int speculation_info(long long out[8]) const;
    // ---- speculation, greedy, SEVERAL conversations in one weight pass.  verify_draft_batch: conversation slots[i] brings its greedy token g0_i and counts[i] draft tokens
    // (drafts: concatenated in list order), i.e. a group of 1 + counts[i] rows at consecutive positions; the groups are packed into one pass of N <= 64 rows
    // (forward_batch's multi mode: the batched step's embedding rows and mat-vec branches at N rows, launch_attn_llm_draft_batched -- causal inside each group --,
    // launch_draft_finish_batch -- one decision per conversation).  g0_i is the conversation's RAW greedy token, verify_draft's rule: penalties, a logit bias and
    // constraints do not enter it, and a row's greedy id is the first maximum of its raw logits.  Per conversation afterwards exactly what verify_draft leaves: ids_out
    // [i][DRAFT_ROWS] = g0_i, draft_i[0 .. m_i), n_out[i] = 1 + m_i, n_past = n_committed = p_i + 1 + m_i, logits / greedy / feed token those of row m_i; row_greedy (may be
    // null) [i][DRAFT_ROWS]: the first argmax of every evaluated row, -1 behind them.  Queued prompt rows of every listed conversation are evaluated first, as decode_batch
    // does.  A draft is cut to the room left; a conversation without room follows decode_batch: the automatic shift makes room, or n_out[i] = 0 and it is left out of
    // the pass, untouched.  One wait per call; commit_rows takes the kept rows only; the sampler's generator, the mirostat state and the prefix store are not touched.
    // (A conversation that still has no logits once its queue is evaluated is refused behind that evaluation: the conversations listed before it keep their evaluated rows.)
    // Every count 0: the ordinary batched step (step_launch(B), its own graph, k_batch_finish) -- that case costs what decode_batch costs.  Parity mode: verify_draft's
    // one-row oracle-order loop per conversation.  Refusals ("verify_draft_batch: ...", nothing changed): speculation off, a bad / duplicate / out-of-range slot list, a
    // count outside [0, max_draft], a token id out of range, a conversation without current logits, more rows in total than the pass holds (64, and the context's
    // activation rows).
    int verify_draft_batch(const int *slots, int n, const int *drafts, const int *counts, int *ids_out, int *n_out, int *row_greedy);
    // decode_lookup's loop over n conversations: each its own NgramDrafter (corpus: concatenated, corpus_counts[i] tokens each, + what it emitted), its own max_tokens
    // budget and its own </s> / context-full end; every iteration is ONE verify_draft_batch over the conversations still running.  tokens_out [n][max_tokens],
    // n_tokens [n], stats [n][4] = {passes in which the conversation sent a draft, passes without one, draft tokens sent, draft tokens accepted}
    int decode_lookup_batch(const int *slots, int n, const int *corpus, const int *corpus_counts, int max_tokens, int ngram_max, int ngram_min, int n_draft, int *tokens_out,
                            int *n_tokens, int *stats);
    // {passes, rows, groups, draft tokens sent, accepted, all-zero calls that took the plain batched step, draft tokens cut for room, 0}; parity mode's one-row loops
    // count nothing here but the cut
    int speculation_batch_info(long long out[8]) const;

    // ---- beam search over forked conversations (beam.hpp: the step's rule; minigpt4_amd.h: the whole rule).  slots[0] is the source, the other n_beams - 1 listed
    // conversations are scratch.  The source's queue is evaluated, its logits row / greedy / feed token saved, its state forked to the others; then every step queues, on one
    // in-order stream and without a host round trip between them, k_topn_rows (top_n = C = 2 n_beams) over the listed logits_ rows, k_beam_select (the W best (beam, token)
    // pairs; it writes the row tokens into d_btok_), the copy of its result block to pinned memory, k_kv_permute (beam i continues from beam parent[i]'s cache rows; over
    // rows [common, position), common = the leading rows known to be equal in all W conversations) and forward_batch at W rows -- the batched step's own pass and graph.  The
    // host awaits the result block while the pass runs and keeps the token ancestry and the finished list.  Afterwards the source is bit for bit what it was (rows below its
    // position are never written; its logits row, greedy and feed token are restored) and the others stand as fork(n_rows = that position) leaves them.  Decisions are on
    // raw logits; sampler, mirostat state, prefix store and every token history are untouched.  Parity mode: the same kernels decide, one oracle-order single-row pass per
    // beam and step evaluates.  stats = {weight passes, k_kv_permute launches whose map was not the identity, cache rows moved (summed over conversations), hypotheses
    // finished by EOS}.  tokens_out: [n_best][max_tokens + 1].  1 + last_error "beam_search: ..." and nothing changed on a refusal.  Buffers: first call; freed with the
    // context and by set_conversations.
    int beam_search(const int *slots, int n_beams, int max_tokens, float length_penalty, int n_best, int *tokens_out, int *lengths_out, float *scores_out, int *n_out, int *stats);
    // ---- guided decoding (classifier-free guidance; minigpt4_amd.h: the rule).  Pair i = the guided conversation pos[i] and the guidance conversation neg[i], all 2 n distinct.
    // Queued rows of all 2 n are evaluated first (prefill_batch over them); then k_guide_rows (one launch) mixes each pair's two logits_ rows and picks.  decode_guided
    // advances BOTH conversations of a pair by the pick through the batched step's own pass and graph (or neither: no room in one of them and no automatic shift).  temp <= 0:
    // a pair whose pos has no bias / penalty takes the pick from the kernel straight into d_btok_ -- the host awaits the ids on an event once the pass is launched --, a pair
    // with one runs k_pen_pick on its mixed row (pos's table) and its id travels through the host.  temp > 0: the mixed rows come to the host in one copy, then penalise_row
    // and the chain, one draw per pair in list order.  Parity mode: the same kernel decides, one oracle-order single-row pass per conversation evaluates.  guided_logits reports
    // the mixed rows (before bias and penalties) and their first maxima and advances nothing.  1 + last_error "end_chat_guided: ..." / "guided_logits: ..." and nothing
    // changed: a bad list, n < 1, 2 n > the conversations, a slot out of range or repeated, a scale that is not finite; after the queued rows: a conversation without current
    // logits.  Buffers: first call; freed with the context and by set_conversations.
    int decode_guided(const int *pos, const int *neg, int n, float scale, const SampleParams &p, int *ids_out);
    int guided_logits(const int *pos, const int *neg, int n, float scale, float *mixed_out, int *pick_out);
    struct GuideInfo { int launches = 0, handed = 0, pen_picked = 0, sampled = 0; };   // k_guide_rows launches; pairs handed to the pass on the device / through k_pen_pick / the host chain
    GuideInfo guidance_info() const { return guide_info_; }
    // ---- repetition / frequency / presence penalties and a logit bias (penalty.hpp: llama.cpp's arithmetic, one definition for host and device).  Off by default
    // (the reference ignores the arguments); minigpt4_amd.h states the rules.  Every conversation keeps a ROW-ALIGNED token history -- entry r = the token id of cache
    // row r, -1 for an embedding row -- that every path which advances or moves rows keeps in step (commit_rows states the invariant; the queued rows
    // follow in pend_tok), its five parameters (neutral by default; they count only while the mode is on) and its bias (counts whatever the mode).  sample_token and
    // decode_batch apply them: temp <= 0 through ONE k_pen_pick launch over the listed conversations whose transformation is not the identity (tables built on the
    // host and staged as pick_stage.hpp describes: one upload, one small copy back, one synchronise; logits_, d_argmax_, d_feed_ and the graphs untouched), temp > 0 on
    // a host copy of the row before the chain.  verify_draft, decode_lookup and decode_loop decide on raw logits.  The staging block is allocated at the first launch.
    void set_penalties(bool on) { pen_mode_ = on; }
    bool penalties() const { return pen_mode_; }
    int set_conversation_penalties(int slot, const PenParams &p);          // 0, or 1 + last_error "conversation_penalties: ...", nothing changed
    int set_logit_bias(const int *ids, const float *bias, int n);          // selected conversation; 0, or 1 + last_error "set_logit_bias: ...", nothing changed
    int token_history(int *out, int cap);                                  // selected conversation, queued rows evaluated first; the count (-1: that pass failed)
    struct PenInfo { int mode = 0, launches = 0, host_rows = 0, last_entries = 0; };
    PenInfo penalty_info() const { PenInfo i = pen_info_; i.mode = pen_mode_; return i; }
    // ---- constrained decoding (constraint.hpp: the pattern language and the DFA; minigpt4_amd.h: the rules).  A compiled constraint belongs to the CONTEXT (handles 1 ..
    // CONSTRAINT_SLOTS; it depends on the vocabulary only, so it survives set_conversations and parity switches): its DFA on the host, and on the device its table and the
    // index k_constrain_index builds once -- the allowed-token bitmap of every state.  A conversation holds a handle (0: none) and a DFA state.  sample_token and
    // decode_batch apply it behind bias and penalties: temp <= 0 through ONE k_constrain_pick launch over the constrained conversations of the call (pen_pick skips them: the
    // kernel applies their tables itself; staged as pick_stage.hpp describes, 4 m bytes come back, one synchronise), temp > 0 by fetching the state's index row and setting every other id of the penalised
    // host copy to -infinity before the chain.  Every constrained pick advances the state by the picked token on the host (EOS leaves it), whether or not the conversation
    // then advances: the state belongs to the sampler, like the generator.  reset() returns it to the start; fork touches neither handle nor state; decode_batch with forced
    // tokens, verify_draft, decode_lookup, decode_loop, beam_search and decode_guided neither consult nor advance it.  The vocabulary blob, the staging block and the
    // indices are allocated by the first compile and freed with the context.  Each call: 0, or 1 + last_error "<name>: ..." and nothing changed.
    static constexpr int CONSTRAINT_SLOTS = 8;
    int constraint_compile(const unsigned char *pattern, long long n_bytes, int *handle);   // n_bytes < 0: strlen
    int constraint_free(int handle);                                       // refused while a conversation holds it
    int set_constraint(int slot, int handle);                              // 0 clears; the state goes to the start
    int constraint_advance(int slot, const int *tokens, int n);            // host walk; a token that leads to state 0 refuses the whole call
    int constraint_info(int slot, int out[8]) const;                       // {handle, state, accepting, n_states, pick launches, host rows, stuck picks, index launches}
    int constraint_mask(int handle, int state, uint32_t *out, int n_words);   // the device index row of (handle, state)

    // ---- sampled batched steps decided on the device (sampling.hpp: the generator and the rule; minigpt4_amd.h: the whole rule).  Every conversation holds a 64-bit seed and
    // a 64-bit count of draws (after init and set_conversations: seed = (uint32)load seed | slot << 32, draws = 0; reset, fork, shift and snapshot loads touch neither: the pair
    // belongs to the sampler, as the host generator does).  decode_batch_sampled is one decode_batch step whose tokens k_sample_rows decides: queued rows of the listed
    // conversations first (one flush each, as decode_batch), then the staging block's one upload (pick_stage.hpp: a SampleRow per conversation + the penalty tables
    // pen_build_row builds), ONE launch over the listed logits_ rows -- a pick goes straight into d_btok_ for every conversation that advances --, the block's fetch (the
    // results to pinned memory + the event), the batched step's own pass (step_begin / step_launch).  The host awaits the event while the pass runs, then does the book-keeping: histories, con_walk, draws += 1 per
    // listed conversation (a full one that cannot shift included: sampled, reported, not advanced).  No logits row travels to the host; no synchronise between decision and
    // pass.  Parity mode: the same kernel decides, the picks are awaited first, step_parity evaluates.  sampled_candidates reports the distribution the next step would draw
    // from (ids [n][64] with -1 behind n_cand, probabilities with 0 behind it) and moves nothing.  1 + last_error "end_chat_batch_sampled: ..." / "sampled_candidates: ..." /
    // "conversation_seed: ..." / "sampling_info: ..." and nothing changed on a refusal (a bad slot list, temp not finite or <= 0, top_k outside 1 .. min(64, n_vocab), top_p
    // outside (0, 1]; after the queued rows: a conversation without current logits).  The host chain and its mt19937 are untouched by all of this.  Buffers: first call;
    // freed with the context and by set_conversations.
    int decode_batch_sampled(const int *slots, int n, float temp, int top_k, float top_p, int *ids_out);
    int sampled_candidates(const int *slots, int n, float temp, int top_k, float top_p, int *ids_out, float *probs_out, int *n_cand_out, int *kept_out);
    int set_conversation_seed(int slot, uint64_t seed, uint64_t draws);
    int sampling_info(int slot, uint64_t out[6]) const;                    // {seed, draws, k_sample_rows launches, picks handed to a pass on the device, stuck picks, rows sampled}
    // ---- the same two calls under the extended rule (sampling.hpp: sample_chain; minigpt4_amd.h states it): tail-free, typical, top-p, min-p, temperature, softmax and
    // the draw over the live list, or mirostat v2 over the candidates.  The steps are decode_batch_sampled's own, one by one (one body: decode_batch_sampled_t), with a
    // staging block of its own kind (SampleRowEx / SampleOutEx, allocated by the first _ex call, freed where smp_ is) and k_sample_rows_ex deciding; the counters of
    // sampling_info count them.  Mirostat's mu is the conversation's, like (seed, draws): NaN = unset, 2 * tau at the first mirostat decision, moved by every
    // decode_batch_sampled_ex decision with mirostat == 2 (the conversation advancing or not), read with the picks from the pinned block; reset, fork, shift and snapshot
    // loads leave it alone, set_conversations unsets it, sampled_candidates_ex does not move it.  Refusals in addition to the plain calls': tfs_z or typical_p outside
    // (0, 1], min_p outside [0, 1], mirostat not 0 or 2 (1: "mirostat v1 is not built"), tau not finite or <= 0, eta not finite or < 0.
    int decode_batch_sampled_ex(const int *slots, int n, float temp, int top_k, float top_p, const ChainParams &cp, int *ids_out);
    int sampled_candidates_ex(const int *slots, int n, float temp, int top_k, float top_p, const ChainParams &cp, int *ids_out, float *probs_out, int *n_cand_out, uint64_t *kept_mask_out);
    int set_conversation_mirostat(int slot, float mu);                     // finite: mu; NaN: unset
    int mirostat_info(int slot, float out[4]) const;                       // {set 0 / 1, mu, last observed surprise, last tau}
    // ---- snapshots (state.hpp: the format; minigpt4_amd.h: the rules).  A conversation leaves its slot, its context or its process as one checksummed blob and comes back
    // bit for bit: cache rows [0, n_rows), token history, logits row, greedy / feed token, penalty parameters and logit bias.  Not in a snapshot: the sampler's generator and
    // mirostat state (context-level), the constraint handle and state (handles are per context), queued rows (a save evaluates them first), the prefix store.
    // The cache travels in blocks of block_rows rows through two device and two pinned staging blocks (allocated by the first save / load, grown when a snapshot's own
    // block size asks for more, freed with the context; they survive set_conversations) and a copy stream of the feature's own: save packs block c + 1 (k_kv_pack, stream_)
    // while block c's device-to-host copy (copy stream) and the host memcpy into the caller's buffer run; load mirrors it (host memcpy, upload, k_kv_unpack).  Every launch
    // leaves its block's checksum in a device word; one small copy fetches them all.  Save writes them into the block table last; load compares them with the table.
    // state_size: the bytes a save of `slot` would take now, queued rows counted (0 + last_error: slot out of range).
    // state_save: 0, or 1 + last_error "state_save: ..." with nothing written and nothing evaluated for a slot out of range or cap < the size (*written = the size needed).
    // state_load: header and every host section are parsed and checked first (fingerprint = n_layer, n_embd, n_head, n_vocab, LLM arena layout hash; n_rows <= n_ctx; ids in
    // range; section sizes) -- a refusal there returns 1 + "state_load: ..." with nothing changed.  Then whatever the slot held, queued rows included, is dropped, the blocks
    // are unpacked and position, device position word, logits row, greedy / feed token, history, penalties and bias installed; the slot's captured decode step stays (the
    // addresses are unchanged, eval_chunk re-captures when the key-split choice differs).  A block whose checksum differs from the table: 1 + "state_load: block c
    // checksum", the conversation left as reset() leaves it -- the one failure that is not "nothing changed".
    size_t state_size(int slot);
    int state_save(int slot, void *buf, size_t cap, size_t *written);
    int state_load(int slot, const void *buf, size_t n);
    struct StateInfo { long long saves = 0, loads = 0, rows_saved = 0, rows_loaded = 0, pack_launches = 0, unpack_launches = 0, checksum_failures = 0, staging_bytes = 0; };
    StateInfo state_info() const { return state_info_; }

    // ---- measurement hooks (bench / tests): both feed tokens back on the device, so the rows they add enter the token history as -1
    // K greedy decode steps fed back on the device (no host round trip); returns ms per step via hipEvents.
    int decode_loop(int steps, int *tokens_out, float *ms_total);
    // Per-launch-site table of the decode step: `steps` eager decode steps issuing EXACTLY the launch set the captured hipGraph replays, a hipEvent
    // pair around every site; JSON array of {site, kernel (symbol as rocprofv3 prints it), calls_per_step, avg_us, bytes_per_call (algorithmic:
    // weight planes / KV rows the site reads)} + the whole-step time.  The events serialise nothing (one in-order stream) but add their own record
    // cost between launches, so the table is for attribution; the step time of record is the graph replay's.
    int profile_sites(int steps, std::string &json);
    float last_encode_ms() const { return last_encode_ms_; }
    void set_parity(bool on);                          // MINIGPT4_PARITY at run time (tests): drops the captured graphs, the next evaluation uses the other mode
    bool parity() const { return parity_; }

private:
    int load_llm(const std::string &path);
    int load_vision(const std::string &path);
    void alloc_buffers();
    void forward_batch(int B, hipStream_t s, bool verify = false, bool epilogue = true, bool multi = false);   // B decode rows of B conversations: tokens d_btok_[r], conversations d_bslot_[r]; verify: of ONE conversation (epilogue = false: without launch_draft_finish); multi: groups of rows of several conversations (verify_draft_batch)
    // speculation's own allocations (set_speculation; freed with the context): [1 + spec_max_][n_vocab] row logits, {m, greedy id per row} and its pinned mirror, [R] graphs
    int spec_max_ = 0; DevPtr<float> spec_logits_; DevPtr<int> spec_res_; PinPtr<int> spec_hres_; std::vector<hipGraphExec_t> spec_graph_;
    // penalties: the penalised pick's staging block (pick_stage.hpp), allocated by the first row that is not the identity; its results are the picked ids
    template <typename Row, typename Out> using Stage = PickStage<Row, Out, MAX_CONVERSATIONS>;
    bool pen_mode_ = false; PenInfo pen_info_;
    Stage<PenRow, int> pen_;
    std::vector<float> pen_row_;                                           // the host path's scratch copy of the row (h_logits_ stays raw)
    // beam search's own lazy allocation: device words [slots 8 | targets 8 | ids 128 | logprobs 128 | rank 8 | target logprob 8 | scores 8 | BeamStep], its pinned mirror
    // (staging of the uploads, the landing place of the result block), the saved logits row + greedy / feed token of the source, the event the result block is awaited on
    DevPtr<int> beam_d_; PinPtr<int> beam_h_; DevPtr<float> beam_save_; OwnedEvent beam_ev_;
    static constexpr int BEAM_IDS = 16, BEAM_LP = BEAM_IDS + BEAM_MAX * BEAM_CAND_MAX, BEAM_RANK = BEAM_LP + BEAM_MAX * BEAM_CAND_MAX, BEAM_TLP = BEAM_RANK + 8, BEAM_S = BEAM_TLP + 8,
                         BEAM_RES = BEAM_S + 8, BEAM_WORDS = BEAM_RES + (int)(sizeof(BeamStep) / 4);
    void beam_alloc();
    void beam_free() { reset_all(beam_d_, beam_h_, beam_save_, beam_ev_); }
    struct Conversation;
    int pen_table(const Conversation &cv, std::vector<PenEntry> &tab) const;   // the conversation's table for its history as a sample sees it; the flags
    // THE row builder of the device picks: cv's bias and penalties over its history as the PenRow of logits row `row` (-> *out, whose entries are to start at entry
    // `off`) and its entries (-> tab).  false: the transformation is the identity (no flags, no entries); *out describes that too, for con_pick, which launches such rows
    bool pen_build_row(const Conversation &cv, int row, size_t off, PenRow *out, std::vector<PenEntry> &tab) const;
    // ... built into row m of pen_ (allocated here), entries at the running offset `off`
    bool pen_stage_row(const Conversation &cv, int row, int m, size_t &off, std::vector<PenEntry> &tab);
    // m staged rows with n_ent entries: the upload, k_pen_pick over rows of `logits`, the ids' copy back queued.  false: the launch was refused (last_error).  Once
    // the caller has synchronised, pen_collect checks the ids and scatters them: ids[map[r]] <- row r's pick
    bool pen_launch(const float *logits, int m, size_t n_ent);
    void pen_collect(int m, const int *map, int *ids) const;
    // THE check of a token id the device reported: the id, or HipError{hipErrorUnknown, what} for one outside the vocabulary.  A caller whose book-keeping has to follow the
    // device before a bad block is reported asks id_in_vocab first and throws bad_id(what) when it is done
    bool id_in_vocab(int id) const { return id >= 0 && id < (int)llm_.n_vocab; }
    static HipError bad_id(const char *what) { return HipError{hipErrorUnknown, what, __FILE__, __LINE__}; }
    int device_id(int id, const char *what) const { if (!id_in_vocab(id)) throw bad_id(what); return id; }
    // THE checks of temp / top_k / top_p of every entry point that samples on the device; false: refuse(...) has set last_error
    template <typename Refuse> bool sampling_params_ok(Refuse refuse, float temp, int top_k, float top_p) const;
    // Every listed conversation has queued rows or current logits; evaluate() runs the queues (the caller's way: the passes it costs differ; false: it failed, last_error
    // says why); then every one has current logits.  false: refuse(...) has set last_error -- before anything ran where a conversation has neither
    template <typename Refuse, typename Evaluate> bool logits_ready(Refuse refuse, const int *slots, int n, Evaluate evaluate);
    // the argument checks decode_lookup and decode_lookup_sampled share, in their order; 0, or 1 with last_error "<name>: ..."
    int lookup_check(const char *name, const int *corpus, int n_corpus, int max_tokens, int ngram_max, int ngram_min, int n_draft, const int *tokens_out, const int *n_tokens,
                     const int *stats) const;
    // THE host chain's bias and penalties (temp > 0), in place on a copy of cv's logits row: bias, then penalties over `hist`; a constraint's mask comes after it
    void pen_host_row(const Conversation &cv, const std::vector<int> &hist, float *row);
    // ids[i] <- the penalised pick of every listed conversation whose transformation is not the identity (skip_constrained: and that holds no constraint -- con_pick serves it)
    void pen_pick(const int *slots, int n, int *ids, bool skip_constrained = true);
    int greedy_raw();                                                      // sample_token at temp 0 without penalties or bias
    void spec_drop_graphs();
    void spec_free();
    // prefill_batch: one packed chunk as forward() sees it through Pass::seg (device tables in d_seg_, host copy of the segment table)
    struct SegChunk {
        int n_seg = 0, n_end = 0;                      // segments; conversations whose queue ends in this chunk
        int h_segs[4 * MAX_CONVERSATIONS];            // [segment][slot, first packed row, rows, position of the first row]
        AttnSegs att;                                  // device segment table + attention work lists
        const int *rows = nullptr, *fin = nullptr, *last = nullptr;   // device: [row][slot, position]; [ending][slot, end position]; [ending] last packed row
        double key_rows = 0;                           // cached rows the segments' attention reads (profile_sites)
    };
    // score request (Pass::score): the pass (forward / forward_ref, plain or packed) also evaluates the output matrix on chunk rows [first, end) and runs k_logprob_rows
    // on them.  targets / logprob / greedy / greedy_logprob: device arrays indexed by chunk row, target -1 = the row predicts nothing that was given; h_logits
    // (plain pass only): host destination of row `first`'s logits, the following rows behind it
    // top_n > 0: k_topn_rows behind k_logprob_rows on every tile, into the top-N result block's score layout (topn_ids() ...), indexed by chunk row
    struct ScoreReq { const int *targets = nullptr; float *logprob = nullptr; int *greedy = nullptr; float *greedy_logprob = nullptr; int first = 0, end = 0; float *h_logits = nullptr;
                      int top_n = 0; };
    // Everything one prompt / decode pass depends on besides the selected conversation.  N rows described by d_tokens_ (id, or -1 = an embedding row already sitting in
    // x_); feed: the decode row, its token taken from d_feed_; split: that row's attention on the key-split launches (decode_pass chooses; no other pass takes them); seg: the rows are a packed chunk of several
    // conversations; score: also score chunk rows [first, end)
    struct Pass { int N; bool feed = false; bool split = false; const SegChunk *seg = nullptr; const ScoreReq *score = nullptr; };
    void forward(const Pass &p, hipStream_t s);
    void forward_ref(const Pass &p, hipStream_t s);    // parity mode: the oracle's accumulation order (never a packed chunk)
    int eval_chunk(const int *row_tok, int N, const float *embd, const ScoreReq *score = nullptr);
    // the request for the chunk rows that have a target (>= 0) in `targets` (one entry per chunk row), uploaded to score_tgt_; end <= first: no row has one, no scoring
    ScoreReq score_request(const std::vector<int> &targets, int top_n, float *h_logits);
    size_t upload_embd_runs(const int *tok, int m, const float *embd, float *x_dst);   // the runs of embedding rows (id -1) among m rows -> their rows of x_dst; rows consumed
    // begin capture, enqueue(), end capture, instantiate; when enqueue() throws the capture is ended (the stream must not stay in capture mode), `out` stays null
    template <class F> void capture_graph(hipGraphExec_t &out, F &&enqueue);
    struct SelectScope { Engine *e; int keep; explicit SelectScope(Engine *e_) : e(e_), keep(e_->cur_) {} ~SelectScope() { e->cur_ = keep; } };   // entry points that walk a slot list with cur_
    int check_slots(const int *slots, int n) const;    // 0; 1: a bad list (null, n < 1, n > the conversations); 2: not distinct / out of range
    void drop_queues(const int *slots, int n) { for (int i = 0; i < n; i++) conv_[(size_t)slots[i]].drop_queue(); }
    // the feature's own lazy allocation (first scoring call; freed with the context): [SCORE_ROWS][n_vocab] logits, and [score_cap_] targets / results -- one per chunk
    // row, then one per conversation for entry 0
    DevPtr<float> score_buf_, score_lp_, score_glp_; DevPtr<int> score_tgt_, score_greedy_; int score_cap_ = 0;
    void score_alloc();
    void score_rows(const ScoreReq &rq, hipStream_t s);
    void score_entry0(int slot, int idx, int target, float *logprob, int *greedy, float *greedy_logprob, float *logits_out, const TopOut *top = nullptr);
    int score_tokens_impl(const char *name, const int *tokens, int n, float *logprob, int *greedy, float *greedy_logprob, float *logits_out, const TopOut *top);
    // the top-N feature's own lazy allocation (first *_top / top_logprobs call; freed with the context): one device block of topn_cap_ * (2 TOPN_MAX + 2) words and its
    // pinned mirror, the slot calls' inputs (row index, target per listed conversation) and the event their copy back is awaited on.  Score passes lay the block out
    // as ids [cap][top_n] | log-probabilities at cap * TOPN_MAX | rank at 2 cap TOPN_MAX | target log-probability behind it; the slot calls pack m rows' ids,
    // log-probabilities, ranks and target log-probabilities back to back from word 0, so that one copy fetches them
    DevPtr<int> topn_d_; PinPtr<int> topn_h_; DevPtr<int> topn_in_; PinPtr<int> topn_hin_; int topn_cap_ = 0; OwnedEvent topn_ev_;
    int topn_map_[MAX_CONVERSATIONS], topn_m_ = 0;                        // the launched rows of the slot call in flight: [row] -> index in the slot list
    int *topn_ids() const { return topn_d_; }
    float *topn_lp() const { return reinterpret_cast<float *>(topn_d_ + (size_t)topn_cap_ * TOPN_MAX); }
    int *topn_rank() const { return topn_d_ + 2 * (size_t)topn_cap_ * TOPN_MAX; }
    float *topn_tlp() const { return reinterpret_cast<float *>(topn_rank() + topn_cap_); }
    void topn_alloc();
    void topn_slots_launch(const int *slots, int n, int top_n, const int *targets);
    void topn_slots_collect(int n, int top_n, int *top_ids, float *top_lp, float *logprob, int *rank);
    struct ScoreOut { int off[MAX_CONVERSATIONS]; float *logprob; int *greedy; float *greedy_logprob; };   // score_batch: [slot] -> the conversation's first output entry
    int prefill_packed(const int *slots, int n, const ScoreOut *so = nullptr);
    void attn_segments(const SegChunk &sg, __half *kc, __half *vc, bool want_h, bool *att_in_xh, hipStream_t s);
    // d_seg_ / h_seg_ layout (ints): segments [0, 256), finish rows [256, 384), last rows [384, 448), row table [448, + 2 max_rows_), then the 16- and 32-query work
    // lists, 2 (max_rows_ + 64) each
    static constexpr int SEG_FIN = 4 * MAX_CONVERSATIONS, SEG_LAST = SEG_FIN + 2 * MAX_CONVERSATIONS, SEG_ROWS = SEG_LAST + MAX_CONVERSATIONS;
    size_t seg_ints() const { return (size_t)SEG_ROWS + 2 * (size_t)max_rows_ + 4 * ((size_t)max_rows_ + MAX_CONVERSATIONS); }
    int *d_seg_ = nullptr, *h_seg_ = nullptr;
    struct Prep { int kind; const float *x; const float *w; };   // 1: rms_norm(x)*w, 2: x, 3: silu(x)*w -- then quantised for the consumer's type
    void mul_mat(const QWeight &W, int N, float *y, int ldy, const float *residual, hipStream_t s, const Prep *prep, bool fuse, const char *site = "matmul", bool defer_ok = false, bool keep_pending = false, bool issue_bar = false);
    bool mul_mat_set(const QWeight *const *W, float *const *y, const float *const *res, int n, int N, int ldy, hipStream_t s, const Prep *prep, bool fuse, bool silu_pair = false, const char *site = "matmul", bool defer_ok = false, bool keep_pending = false, bool issue_bar = false);
    // prompt passes: the combine of a K-split mat-mul is left to the kernel that consumes the result (rope + cache append, the next norm +
    // quantisation, silu * mul); pend_ describes the slabs until then, flush_pending runs the combine as its own launch when the next consumer is not
    // one of those.  MINIGPT4_DEFER_COMBINE=0: always flush (A/B)
    SlabSrc pend_; bool defer_combine_ = true;
    const __half *xh_override_ = nullptr; int f16_pair_ = 7;   // F16 prompt pass: w1 | w3 + silu * mul in one launch, its fp16 rows feed w2 (MINIGPT4_F16_PAIR=0: A/B)
    // batched decode of > batch_rows_max_ conversations through the prompt pass's set launches (MINIGPT4_BATCH_SETS=0: one launch per matrix, A/B)
    bool batch_sets_ = true;
    void flush_pending(hipStream_t s);
    void prep_rms(const float *x, const float *w, int N, int K, int mask, hipStream_t s);
    void upload_qweight(const TensorMeta &t, const uint8_t *file_base, QWeight &w);
    template <typename T> T *upload_raw(DeviceArena &a, const void *src, size_t bytes);


    int native_broadcast(int world, int rank, const std::string &id_file, int timeout_s, int local_err = 0);
    int dist_world_ = 1, dist_rank_ = 0; float dist_bcast_ms_ = 0.0f;
    LoadMode load_mode_ = LOAD_FULL;
    bool moves_data() const { return load_mode_ == LOAD_FULL; }
    bool weights_missing() const;      // LOAD_RECV before weights_received(): sets the error text, true
    int device_ = 0;
    hipStream_t stream_ = nullptr;
    int n_ctx_ = 2048, n_batch_ = 512, max_rows_ = 512;
    struct Conversation {
        int n_past = 0;        // logical position: evaluated + queued rows
        int n_committed = 0;   // rows already evaluated on the device
        std::vector<int> pend_tok; std::vector<float> pend_embd;
        hipGraphExec_t graph = nullptr;   // decode step captured with this conversation's cache / position / token addresses
        bool graph_split = false;         // ... with the key-split attention launches (long context) or the one-workgroup-per-head kernel
        std::vector<int> hist;            // token id of every evaluated row, -1 = embedding row / fed back on the device (commit_rows)
        PenParams pen; std::vector<int> bias_id; std::vector<float> bias_val;   // penalties (while the mode is on), logit bias (always)
        bool has_logits = false;          // its logits_ row holds the logits after its last evaluated row (not: nothing evaluated yet, after reset(), after a partial fork)
        void drop_queue() { pend_tok.clear(); pend_embd.clear(); n_past = n_committed; }   // what a failed pass, fork and reset leave: nothing queued
    };
    std::vector<Conversation> conv_ = std::vector<Conversation>(1);
    // The decode step of a conversation.  Long contexts: its attention shares every head's keys between workgroups (two launches instead of one: pays from a few hundred
    // keys on).  The choice is part of the captured graph, so a conversation that crosses the threshold gets its step re-captured (once).
    Pass decode_pass(const Conversation &cv, const ScoreReq *score = nullptr) const { Pass p{1, true, attn_split_t_ > 0 && cv.n_committed + 1 > attn_split_t_}; p.score = score; return p; }
    int cur_ = 0;
    int shift_keep_ = -1;                  // set_context_shift
    // prefix store: its own allocations (set_conversations re-takes buf_arena_, the store is only emptied then); pfx_ids_.size() = stored rows
    DevPtr<__half> pfx_k_, pfx_v_; int pfx_max_ = 0; std::vector<int> pfx_ids_; PrefixInfo pfx_;
    void prefix_empty() { pfx_ids_.clear(); }
    void prefix_free();
    static int token_run(const Conversation &cv) { int r = 0; while (r < (int)cv.pend_tok.size() && cv.pend_tok[(size_t)r] >= 0) r++; return r; }
    // The store's part of one flush (n = 1) / packed prefill (n > 1).  prefix_lookup: m[i] = rows conversation slots[i] takes from the store (0: none, not at position 0,
    // nothing queued, store off) -- copied in by one launch, n_committed = m[i]; prefix_commit, once every chunk succeeded: the counters, then the capture
    struct PrefixPlan { int m[MAX_CONVERSATIONS] = {0}, hit[MAX_CONVERSATIONS], n_hit = 0, rows = 0, reused = 0; bool looked = false; int cap_slot = -1; std::vector<int> cap_ids; };
    PrefixPlan prefix_lookup(const int *slots, int n);
    void prefix_commit(const PrefixPlan &plan);
    void prefix_copy_in(const int *slots, int n, int n_rows);   // store -> the listed conversations' caches, one launch
    void prefix_capture(int slot, const std::vector<int> &ids);   // that conversation's rows [0, ids.size()) -> store
    bool shift_allows(int n) const { return shift_keep_ >= 0 && n <= n_ctx_ - shift_keep_; }   // the policy is on and n more rows fit behind the kept ones
    int make_room(int n);                  // the automatic shift for n more rows of the selected conversation: 0 = room made (or already there), 1 = not
    bool defer_ = true; int max_chunk_ = 512;
    void release_buffers();

    // LLM
    LLMFile llm_;
    Tokenizer tok_;
    Sampler sampler_;
    struct LayerW { float *attn_norm = nullptr, *ffn_norm = nullptr; QWeight wq, wk, wv, wo, w1, w2, w3; };
    bool mixed_qkv(const LayerW &L, hipStream_t s, bool fuse);
    std::vector<LayerW> layers_;
    float *norm_ = nullptr;
    QWeight output_;
    uint8_t *tok_raw_ = nullptr; int tok_type_ = -1;
    DeviceArena llm_arena_, vis_arena_, buf_arena_;
    // a collective of the native broadcast never completed (a peer died inside it): the stream will not drain, so the destructor must neither wait for it nor free
    // anything queued work may still touch -- the context's device memory is leaked, the load fails, the process lives
    bool stream_hung_ = false;
    uint8_t *stage_ = nullptr; size_t stage_cap_ = 0;
    size_t wbytes_token_ = 0;
    __half *kc_ = nullptr, *vc_ = nullptr;
    float *cos_ = nullptr, *sin_ = nullptr;
    Tables tabs_;
    // tabs_ = ggml's three fp16 tables (GELU, SiLU, exp) as the host libm evaluates them: what parity mode, the quantised models' prompt passes, prompt-row attention, the decode
    // mat-vec's fused SiLU prologue / pair epilogue and the stand-alone GELU epilogue launch read.
    // tabs_dec_ = what the DECODE step's attention and its stand-alone SiLU preparation launch get (and, pair_silu_computed_, the F16 model's w1 | w3 pair launch, which serves prompt
    // chunks from 512 rows up -- shorter chunks gather); tabs_vis_ = what the ViT / Q-Former attention and the vision GEMMs' GELU epilogues get: copies of tabs_ whose exp / silu resp.
    // exp / gelu (computed_gelu_) pointers are NULL when MINIGPT4_COMPUTED_TABLES is on (the default) -- the kernels then compute the table VALUES (activations.hpp exp_h / silu_h /
    // gelu_h; within one fp16 ulp of the table on every argument, recorded on an MI355X: 0 / 2 / 1 of 63 488 arguments different) instead of gathering them from the 128 KB tables
    Tables tabs_dec_, tabs_vis_;
    // activations
    float *x_ = nullptr, *q_ = nullptr, *k_ = nullptr, *v_ = nullptr, *att_ = nullptr, *h1_ = nullptr, *h3_ = nullptr, *logits_ = nullptr;
    ActQ act_;
    // per conversation (indexed by slot): position, greedy token of the last evaluation, next input token; logits_ is [slots][n_vocab]
    int *d_npast_ = nullptr, *d_argmax_ = nullptr, *d_feed_ = nullptr;
    int *d_tokens_ = nullptr; void *d_scratch_ = nullptr;
    // batched decode: row tokens / conversations / positions (one slab, BSTAGE_BYTES), [rows][n_vocab] logits
    int *d_btok_ = nullptr, *d_bslot_ = nullptr, *d_bpos_ = nullptr; float *blogits_ = nullptr;
    // [B]: the batched step for B rows.  The rows are described in device memory, so ONE graph serves every set of B conversations and every entry point that
    // advances B rows (decode_batch, beam_search, decode_guided): all of them launch it through step_launch and nowhere else
    std::vector<hipGraphExec_t> batch_graph_;
    // ---- the batched step, issued in one place.  The slab: [tokens | conversations | positions], MAX_CONVERSATIONS ints each (768 bytes), pinned in h_bstage_ and
    // mirrored by d_btok_ | d_bslot_ | d_bpos_; only these members know the layout.  The caller has synchronised since the slab's last copy was queued.
    static constexpr size_t BSTAGE_BYTES = 3 * (size_t)MAX_CONVERSATIONS * sizeof(int);
    void stage_row(int r, int token, int slot, int position) { h_bstage_[r] = token; h_bstage_[MAX_CONVERSATIONS + r] = slot; h_bstage_[2 * MAX_CONVERSATIONS + r] = position; }
    int &staged_token(int r) { return h_bstage_[r]; }
    int staged_slot(int r) const { return h_bstage_[MAX_CONVERSATIONS + r]; }
    // the slab's one copy, then k_batch_begin over B rows (verify: k_draft_begin -- R rows of the one conversation in row 0)
    void step_begin(int B, bool verify = false, bool multi = false);
    // the weight pass over the staged rows, forward_batch(B, stream_, verify, epilogue): batch_graph_[B] (verify: spec_graph_[B]; verify without its epilogue, the sampled
    // verify pass: spec_sgraph_[B]) replayed, captured first where it does not exist yet; without graphs, eager
    // multi (verify_draft_batch): mspec_graph_[B], B the TOTAL row count -- the grouping is data in d_bslot_ / d_bpos_, so one graph serves every grouping
    void step_launch(int B, bool verify = false, bool epilogue = true, bool multi = false);
    // parity mode's stand-in for step_begin + step_launch: one oracle-order single-row pass per staged row, in row order; cur_ is left on the last row's conversation.
    // 0, or eval_chunk's failure
    int step_parity(int B);
    // THE book-keeping after conversation `slot` had n more rows with these ids evaluated: the history grows by them (invariant: hist.size() == n_committed, the
    // queued rows follow in pend_tok), its logits_ row is current, the host copy of that row is stale.  past: n_past follows too (a caller that had counted the rows
    // into n_past when it queued them passes false)
    void commit_rows(int slot, const int *ids, int n, bool past);
    int *h_argmax_ = nullptr, *h_bstage_ = nullptr; float *h_logits_ = nullptr; int logits_host_slot_ = -1;
    bool use_graph_ = true, use_v2_ = true, attn_prefill_ = true, parity_ = false;
    FILE *trace_file_ = nullptr;       // MINIGPT4_PARITY_TRACE
    // key-split decode attention (llm_kernels.hip: k_attn_split_*)
    void *attn_ws_ = nullptr; int attn_splits_ = 6; int attn_split_t_ = 768; int attn_splits_forced_ = 0;
    // value-column split of the one-row decode attention (k_attn_llm's VS; MINIGPT4_ATTN_VS; 0 = chosen at the launch).  The batched and the verify pass stay at 1
    int attn_vs_ = 0;
    // issue barrier of the decode step's prologue mat-vec launches (kernels.hpp: issue_bar), one default per launch site: on where it won on the 13B Q5_K_M step (per
    // launch 17.64 -> 17.13 us qkv and w1|w3, 14.03 -> 13.60 mixed qkv, 24.88 -> 24.77 output), off for wo (6.99 -> 7.13 us: its two or three row groups per wave leave
    // nothing to reorder); profiles/r13_matvec_prefetch_depth.log.  MINIGPT4_MV_IB = 0 / 1 forces it off / on at every site
    enum MvSite { MV_QKV = 0, MV_QKV_MIXED, MV_WO, MV_W1W3, MV_OUTPUT, MV_SITES };
    bool mv_issue_bar_[MV_SITES] = {true, true, false, true, true};
    int batch_rows_max_ = 4; int batch_fuse_ = -1;
    LaunchTuning tune_;   // CU count + launch switches of THIS context (launch_tuning_from_env in init); passed to every launcher that chooses a grid or a kernel form
    // round 5: B = 2..4 rows per weight pass on the int8 matrix cores over a row-interleaved second image of the k-quant matrices (ri_kernels.hip);
    // built by set_conversations(n > 1) -- a context with one conversation never pays the memory.  MINIGPT4_RI=0: the v_dot4 multi-row mat-vec of
    // rounds 2-4 (A/B)
    bool computed_tables_ = true;
    bool pair_silu_computed_ = true;   // the F16 model's w1 | w3 pair epilogue computes the SiLU table's values (with computed_tables_; MINIGPT4_PAIR_SILU_COMPUTED=0: gathers; round 6)
    bool computed_gelu_ = true;        // with computed_tables_: the vision GEMMs' GELU epilogues compute the table's values too (round 6)
    // B = 4: w2 (80 row groups x long K) on the K-split form of k_matvec_ri (+1.9 %; MINIGPT4_RI_W2=0: the v_dot4 launch)
    bool ri_w2_ = true;
    bool ri_wo_ = false;               // MINIGPT4_RI_WO (round 6 experiment): wo on k_matvec_ri with the plain row quantisation in its prologue
    // ri_fuse_: rows prepared inside the MFMA launches -- measured slower (profiles/r05_batched_decode_inengine.log), off
    bool use_ri_ = true, ri_ready_ = false, ri_fuse_ = false;
    DeviceArena ri_arena_;
    BatchPath batch_path_;
    RiWorkspace ri_ws_;                                     // this context's K-split workspace of k_matvec_ri (slabs + zeroed tickets; passed with every launch)
    std::vector<std::pair<const QWeight *, RiPlanes>> ri_map_;
    const RiPlanes *ri_of(const QWeight *w) const { for (const auto &e : ri_map_) if (e.first == w) return &e.second; return nullptr; }
    void build_ri_planes();
    // MINIGPT4_BATCH_MIX=0: wq|wk and wv of a mixed-type layer as two launches (the form before k_matvec_tn_mix)   // MINIGPT4_BATCH_ROWS_MAX:
    // batches up to this size use the multi-row mat-vec; 0 = never.  Measured (profiles/r02x_*): from 5 rows on the int8-MFMA kernels (single-wave
    // workgroups, one token tile) beat two passes of the 4-row mat-vec
    bool batch_mix_ = true;
    static constexpr int FUSE_DEFAULT = 87; int fuse_mask_ = FUSE_DEFAULT;
    // profiling (profile_sites)
    bool prof_on_ = false;
    struct SiteEv { hipEvent_t a, b; const char *site; std::string kernel; double bytes; size_t p0 = 0, p1 = 0; };   // [p0, p1): the launch probes of the site
    std::vector<SiteEv> site_events_;
    void site_begin(const char *site, double bytes, hipStream_t s);
    void site_end(hipStream_t s) noexcept;
    struct SiteScope { Engine *e; hipStream_t s; SiteScope(Engine *e_, const char *site, double bytes, hipStream_t s_) : e(e_), s(s_) { e->site_begin(site, bytes, s); } ~SiteScope() { e->site_end(s); } };

    // vision
    VisionFile vis_;
    int v_D_ = 0, v_depth_ = 0, v_M_ = 0, v_heads_ = 0, v_ql_ = 0, v_qi_ = 0, v_nq_ = 32, v_out_ = 0;
    struct VBlock { float *n1w, *n1b, *n2w, *n2b, *qkv_b, *proj_b, *fc1_b, *fc2_b; __half *qkv_w, *proj_w, *fc1_w, *fc2_w; };
    struct QAtt { __half *q_w = nullptr, *kv_w = nullptr, *dense_w = nullptr; float *q_b = nullptr, *kv_b = nullptr, *dense_b = nullptr, *ln_w = nullptr, *ln_b = nullptr; };
    struct QLayer { QAtt self, cross; bool has_cross = false; int cross_idx = -1; __half *inter_w, *out_w; float *inter_b, *out_b, *oln_w, *oln_b; };
    std::vector<VBlock> vblocks_;
    std::vector<QLayer> qlayers_;
    float *v_cls_ = nullptr, *v_pos_ = nullptr, *v_patch_b_ = nullptr, *v_lnv_w_ = nullptr, *v_lnv_b_ = nullptr, *v_qtok_ = nullptr, *v_qeln_w_ = nullptr, *v_qeln_b_ = nullptr, *v_proj_b_ = nullptr;
    __half *v_patch_w_ = nullptr, *v_proj_w_ = nullptr;
    // vision activations
    static constexpr int SPLITK_MAX = 12; int splitk_proj_ = 1, splitk_fc2_ = 4;   // MINIGPT4_SPLITK=proj,fc2 (1 = off)
    float *vi_slab_ = nullptr, *vi_qtok_rep_ = nullptr;
    float *vi_img_ = nullptr, *vi_pe_ = nullptr, *vi_x_ = nullptr, *vi_qkv_ = nullptr, *vi_hs_ = nullptr, *vi_a1_ = nullptr, *vi_a2_ = nullptr, *vi_d_ = nullptr, *vi_qq_ = nullptr, *vi_kv_ = nullptr, *vi_out_ = nullptr;
    __half *vi_patches_ = nullptr, *vi_ln_h_ = nullptr, *vi_att_h_ = nullptr, *vi_mlp_h_ = nullptr, *vi_img_h_ = nullptr, *vi_hs_h_ = nullptr, *vi_a1_h_ = nullptr, *vi_a2_h_ = nullptr, *vi_ctx_h_ = nullptr, *vi_im_h_ = nullptr;
    float last_encode_ms_ = 0;
    bool qf_skinny_ = true;            // Q-Former GEMMs on k_gemm_f16_skinny
    // round 5, launch count of the image path: (1) the cross-attention K | V projections of ALL cross layers are one weight block [n_cross * 1536][D]
    // -- they depend on the image features only (minigpt4.cpp:1148-1155), so one GEMM right after ln_vision replaces one per cross layer; (2) what
    // the Q-Former computes BEFORE it first looks at the image -- LayerNorm(query tokens), layer 0's self-attention block and its cross-attention
    // query projection -- does not depend on the image at all: evaluated once at load time by the same launches (fold_qformer_constants), kept for
    // every image of a batch.  MINIGPT4_QF_FOLD=0 / MINIGPT4_KV_HOIST=0: the round-4 form (A/B).
    __half *v_kv_all_w_ = nullptr; float *v_kv_all_b_ = nullptr; int v_ncross_ = 0;
    float *vi_c_a1_ = nullptr, *vi_c_qq_ = nullptr; __half *vi_c_a1_h_ = nullptr;
    bool qf_fold_ = true, qf_folded_ = false, kv_hoist_ = true;
    void fold_qformer_constants();
    bool qf_splitk_ = true;
    bool qkv_head_major_ = true;       // the ViT's qkv projection stores q | k | v head-major for k_attn_vit (round 6)
    void qf_dense_ln(const __half *A, int lda, const __half *W, int K, const float *bias, const float *residual, const float *ln_w, const float *ln_b, float *out, __half *out_h,
                     int rows, hipStream_t s);

    // ---- vision files whose Linear weights are not all F16 (an `--ftype f32` conversion, or a file written by minigpt4_quantize_model): every
    // Linear is a QWeight served by the LLM mat-mul kernels (activations quantised to the weight type's vec_dot_type, exactly ggml's mul_mat),
    // activations stay fp32.
    bool v_generic_ = false;
    struct GLin { QWeight w; };
    struct GBlock { GLin qkv, proj, fc1, fc2; };
    struct GAtt { GLin q, k, v, dense; };
    struct GQLayer { GAtt self, cross; GLin inter, out; };
    std::vector<GBlock> gblocks_; std::vector<GQLayer> gql_; GLin gproj_;
    DeviceArena vgen_arena_;
    ActQ vact_;
    float *vg_ln_ = nullptr, *vg_att_ = nullptr, *vg_mlp_ = nullptr, *vg_img_ = nullptr, *vg_tmp_ = nullptr, *vg_ctx_ = nullptr, *vg_im_ = nullptr;
    int load_vision_generic();
    void alloc_vision_generic();
    int encode_images_generic(const float *const *chw, int B, float *const *out);
    int encode_images_ref(const float *const *chw, int B, float *const *out);   // parity mode (engine_vision_generic.cpp)
    void build_vision_views();
    void glinear(const GLin &L, const float *x, int rows, const float *bias, bool gelu, const float *residual, float *out, hipStream_t s);
    // (behind everything else: the members every other path reads lie where they lay before the feature)
    // guided decoding's own lazy allocation: the mixed rows [GUIDE_MAX][n_vocab]; device words [pair table 8 x 32 | picks 32 | pick values 32] and the pinned mirror (staging of
    // the table, landing place of the picks); the event the picks are awaited on; the host copy of the mixed rows (temp > 0, guided_logits)
    DevPtr<float> guide_mix_; DevPtr<int> guide_d_; PinPtr<int> guide_h_; OwnedEvent guide_ev_; std::vector<float> guide_rows_; GuideInfo guide_info_;
    static constexpr int GUIDE_PICK = 8 * GUIDE_MAX, GUIDE_VAL = GUIDE_PICK + GUIDE_MAX, GUIDE_WORDS = GUIDE_VAL + GUIDE_MAX;
    void guide_alloc();
    void guide_free() { reset_all(guide_mix_, guide_d_, guide_h_, guide_ev_); }
    int guide_prepare(const char *name, const int *pos, const int *neg, int n, float scale, int *all);   // the checks, the queued rows; all[2 i] = pos[i], all[2 i + 1] = neg[i]
    // constrained decoding.  Per compiled constraint: the host DFA, the device table | accepting bitmap | index (one allocation).  Per conversation (arrays here, not in
    // Conversation: that struct keeps its layout): handle and state.  Lazy, first compile: the vocabulary blob + offsets; the pick's staging block (pick_stage.hpp; its
    // results are the output words), the pinned landing place of one index row (temp > 0, constraint_mask)
    struct Constraint { bool used = false; ConstraintDfa dfa; DevPtr<uint8_t> dev; const unsigned *index = nullptr; };
    Constraint con_[CONSTRAINT_SLOTS];
    int con_handle_[MAX_CONVERSATIONS] = {0}, con_state_[MAX_CONVERSATIONS] = {0}, con_assigned_ = 0;
    struct ConInfo { int launches = 0, host_rows = 0, stuck = 0, index_launches = 0; } con_info_;
    DevPtr<unsigned char> con_vocab_; DevPtr<int> con_off_;
    Stage<ConRow, int> con_stage_; PinPtr<unsigned> con_row_h_;
    void con_alloc();
    void con_walk(int slot, int id);                                       // the state after the picked token (EOS and ids outside the vocabulary leave it)
    void con_pick(const int *slots, int n, int *ids);                      // ids[i] <- the constrained pick of every listed conversation that holds a constraint
    const unsigned *con_fetch_row(int handle, int state);                  // index[state] of that constraint in con_row_h_, synchronised
    // snapshots' own lazy allocation (first state_save / state_load; freed with the context, kept by set_conversations): two device and two pinned staging blocks of
    // state_cap_ bytes each; one checksum word per block of a snapshot (at most n_ctx blocks) + one word for the greedy | feed token, device and pinned; the copy stream;
    // per staging block the event behind its kernel (stream_) and behind its copy (copy stream).  state_block_bytes_: MINIGPT4_STATE_BLOCK_BYTES (read by init)
    DevPtr<__half> state_d_[2]; PinPtr<uint8_t> state_h_[2]; DevPtr<unsigned long long> state_sum_d_; PinPtr<unsigned long long> state_sum_h_;
    OwnedStream state_cs_; OwnedEvent state_ev_kernel_[2], state_ev_copy_[2];
    size_t state_cap_ = 0, state_sum_words_ = 0, state_block_bytes_ = STATE_BLOCK_BYTES_DEFAULT;
    StateInfo state_info_;
    void state_alloc(size_t block_bytes);              // staging for blocks of that size (all or nothing; grows, never shrinks)
    int state_header(int slot, StateHeader &h, StateLayout &l) const;   // what a save of `slot` would write now (n_rows = n_past); 0, or 1: the layout refused
    // device-side sampling.  Per conversation (arrays here, not in Conversation: that struct keeps its layout): seed and draws.  Lazy, first call: the staging block
    // (pick_stage.hpp); its results are the SampleOut blocks, awaited on its event
    uint64_t smp_seed_[MAX_CONVERSATIONS] = {0}, smp_draws_[MAX_CONVERSATIONS] = {0}; uint32_t smp_load_seed_ = 0;
    struct SmpInfo { uint64_t launches = 0, handed = 0, stuck = 0, rows = 0; } smp_info_;
    Stage<SampleRow, SampleOut> smp_;
    // the extended rule: its staging block (first _ex call) and, per conversation, mirostat's mu (NaN: unset), the last observed surprise and the tau it was measured against
    Stage<SampleRowEx, SampleOutEx> smpx_;
    float smp_mu_[MAX_CONVERSATIONS], smp_observed_[MAX_CONVERSATIONS] = {0}, smp_tau_[MAX_CONVERSATIONS] = {0};
    template <bool EX> auto &smp_block() { if constexpr (EX) return smpx_; else return smp_; }
    static SampleRow &smp_plain(SampleRow &r) { return r; }
    static SampleRow &smp_plain(SampleRowEx &r) { return r.base; }
    static const SampleOut &smp_plain(const SampleOut &o) { return o; }
    static const SampleOut &smp_plain(const SampleOutEx &o) { return o.base; }
    void smp_free() { smp_.reset(); smpx_.reset(); }
    void smp_reseed() {
        for (int s = 0; s < MAX_CONVERSATIONS; s++) { smp_seed_[s] = (uint64_t)smp_load_seed_ | (uint64_t)s << 32; smp_draws_[s] = 0; smp_mu_[s] = NAN; smp_observed_[s] = smp_tau_[s] = 0.0f; }
    }
    // the checks and the queued rows of the entry points; 0, or 1 with last_error "<name>: ..."; cp (the _ex calls): its ranges, behind top_p's
    int smp_prepare(const char *name, const int *slots, int n, float temp, int top_k, float top_p, const ChainParams *cp = nullptr);
    // THE descriptor of one decision of conversation `slot`: its seed, the table `pen` describes, the allowed bitmap of constraint state `state` (no constraint: every id),
    // draw number `draws`; tok_index: the entry of d_btok_ that takes the pick (-1: none)
    SampleRow smp_row(int slot, const PenRow &pen, int state, uint64_t draws, int tok_index, float temp, int top_k, float top_p) const;
    // the listed conversations' descriptors into the block (allocated here; row-token index -1), from each history as a sample sees it; the table entries staged.
    // EX: the block is smpx_, every descriptor carries *cp and its conversation's mu
    template <bool EX = false> size_t smp_stage(const int *slots, int n, float temp, int top_k, float top_p, const ChainParams *cp = nullptr);
    // n staged descriptors with n_ent entries: the upload and the launch over rows of `logits` (row_tok: picks go there at the descriptors' row-token indices), nothing
    // counted, no copy back (verify_draft_sampled: its launches are speculation_info's).  false: the launch was refused (last_error)
    template <bool EX = false> bool smp_launch_on(const float *logits, int n, size_t n_ent, int *row_tok = nullptr);
    // ... over logits_ (hand: picks go to d_btok_), counted, the result block's copy back and the event queued
    template <bool EX = false> bool smp_launch(int n, size_t n_ent, bool hand);
    // THE sampled step and THE report of what it would draw from, under the plain rule (EX false: cp unused) or the extended one
    template <bool EX> int decode_batch_sampled_t(const char *name, const int *slots, int n, float temp, int top_k, float top_p, const ChainParams *cp, int *ids_out);
    template <bool EX> int verify_draft_sampled_t(const int *draft, int n_draft, float temp, int top_k, float top_p, const ChainParams *cp, int *ids_out, int *n_out, int *next_out,
                                                  int *row_sampled, float *row_logits, const char *name, int *n_sent);
    template <bool EX> int decode_lookup_sampled_t(const int *corpus, int n_corpus, int max_tokens, int ngram_max, int ngram_min, int n_draft, float temp, int top_k, float top_p,
                                                   const ChainParams *cp, int *tokens_out, int *n_tokens, int *stats);
    template <bool EX> int sampled_candidates_t(const char *name, const int *slots, int n, float temp, int top_k, float top_p, const ChainParams *cp, int *ids_out, float *probs_out,
                                                int *n_cand_out, int *kept_out, uint64_t *kept_mask_out);
    // speculation under sampling.  Lazy, first call: one graph slot per row count (the verify pass without its epilogue), the result block {m, picks, stuck flags} and its
    // pinned mirror.  Dropped / freed where the greedy form's are (spec_drop_graphs, spec_free)
    std::vector<hipGraphExec_t> spec_sgraph_; DevPtr<int> sdr_res_; PinPtr<int> sdr_hres_;
    // the verify pass of several conversations (verify_draft_batch): its own lazy allocation (first call; freed by spec_free) -- [ATTN_MDRAFT_ROWS][n_vocab] row logits, the
    // result block m [ATTN_MDRAFT_ROWS] | row_greedy [ATTN_MDRAFT_ROWS] and its pinned mirror, one graph per total row count (dropped by spec_drop_graphs)
    DevPtr<float> mspec_logits_; DevPtr<int> mspec_res_; PinPtr<int> mspec_hres_; std::vector<hipGraphExec_t> mspec_graph_;
    void mspec_alloc();
    struct SpecBatchInfo { long long passes = 0, rows = 0, groups = 0, sent = 0, accepted = 0, plain = 0, cut = 0; } mspec_info_;
    struct SpecInfo { long long passes = 0, rows = 0, sent = 0, accepted = 0, launches = 0, stuck = 0, cut = 0; } spec_info_;
    void sdr_alloc();
};

int device_count_noexcept();

// minigpt4_preprocess_image on the device (reference minigpt4.cpp:2597-2651): u8 HWC RGB of any size -> f32 [3][224][224], Pillow-bicubic resized and
// CLIP-normalised.  Host buffers in and out; the resample + normalisation run as HIP kernels on `s`.  Throws HipError.
void preprocess_image_device(hipStream_t s, const uint8_t *rgb, int w, int h, float *out_chw);

}  // namespace mg4
