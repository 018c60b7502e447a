#include "engine.hpp"
#include "dist.hpp"
#include "draft.hpp"
#include "draft_host.hpp"
#include "beam_host.hpp"
#include "quantize.hpp"
#include "imageio.hpp"

#include <algorithm>
#include <optional>
#include <unistd.h>
#include <chrono>
#include <thread>
#include <cmath>
#include <cstring>

namespace mg4 {

// ====================================================================================================================
// device helpers
// ====================================================================================================================
int device_count_noexcept() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}
void DeviceArena::alloc(size_t bytes) {
    release();
    if (virt) base = reinterpret_cast<uint8_t *>((uintptr_t)1 << 40);      // never dereferenced
    // alignment gaps / plane padding are part of what arena checksums cover: make them deterministic
    else { HIP_CHECK(hipMalloc((void **)&base, bytes)); HIP_CHECK(hipMemset(base, 0, bytes)); HIP_CHECK(hipDeviceSynchronize()); }
    cap = bytes; used = 0; layout_hash = 1469598103934665603ull;
}
void DeviceArena::release() { if (base && !virt) HIP_IGNORE(hipFree(base)); base = nullptr; cap = used = 0; }
uint8_t *DeviceArena::take(size_t bytes, size_t align) {
    const size_t off = (used + align - 1) / align * align;
    if (off + bytes > cap) throw HipError{hipErrorOutOfMemory, "arena overflow", __FILE__, __LINE__};
    used = off + bytes;
    for (uint64_t v : {(uint64_t)off, (uint64_t)bytes}) for (int i = 0; i < 8; i++) { layout_hash ^= (v >> (8 * i)) & 0xFF; layout_hash *= 1099511628211ull; }
    return base + off;
}
template <typename T> T *Engine::upload_raw(DeviceArena &a, const void *src, size_t bytes) {
    uint8_t *d = a.take(bytes);
    if (moves_data()) HIP_CHECK(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
    return reinterpret_cast<T *>(d);
}

// ====================================================================================================================
// image preprocess (standalone: needs a device, not a loaded model)
// ====================================================================================================================
void preprocess_image_device(hipStream_t s, const uint8_t *rgb, int w, int h, float *out_chw) {
    constexpr int OUT = 224;                                                   // IMAGE_RESIZE (reference minigpt4.cpp:2620)
    const float mean[3] = {(float)0.48145466, (float)0.4578275, (float)0.40821073}, sd[3] = {(float)0.26862954, (float)0.26130258, (float)0.27577711};   // :2621-2622
    // Pillow skips a pass that keeps the size; an identity table (one tap of 2^22) is the same thing: (2^21 + p * 2^22) >> 22 == p
    auto table = [&](int in, ResampleCoeffs &c) {
        if (in != OUT) { precompute_bicubic_8bpc(in, OUT, c); return; }
        c.in_size = c.out_size = OUT; c.ksize = 1; c.first.resize(OUT); c.count.assign(OUT, 1); c.kk.assign(OUT, 1 << 22);
        for (int i = 0; i < OUT; i++) c.first[(size_t)i] = i;
    };
    ResampleCoeffs ch, cv;
    table(w, ch); table(h, cv);
    struct Dev { void *p = nullptr; ~Dev() { if (p) HIP_IGNORE(hipFree(p)); } };
    Dev d_src, d_tmp, d_out, d_tab;
    const size_t src_bytes = (size_t)w * h * 3, tmp_bytes = (size_t)h * OUT * 3, out_bytes = (size_t)3 * OUT * OUT * 4;
    std::vector<int> tab;                                                      // [first_h | count_h | kk_h | first_v | count_v | kk_v]
    tab.insert(tab.end(), ch.first.begin(), ch.first.end()); tab.insert(tab.end(), ch.count.begin(), ch.count.end()); tab.insert(tab.end(), ch.kk.begin(), ch.kk.end());
    const size_t voff = tab.size();
    tab.insert(tab.end(), cv.first.begin(), cv.first.end()); tab.insert(tab.end(), cv.count.begin(), cv.count.end()); tab.insert(tab.end(), cv.kk.begin(), cv.kk.end());
    HIP_CHECK(hipMalloc(&d_src.p, src_bytes)); HIP_CHECK(hipMalloc(&d_tmp.p, tmp_bytes)); HIP_CHECK(hipMalloc(&d_out.p, out_bytes)); HIP_CHECK(hipMalloc(&d_tab.p, tab.size() * 4));
    HIP_CHECK(hipMemcpyAsync(d_src.p, rgb, src_bytes, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
    const int *t = static_cast<const int *>(d_tab.p);
    launch_resample_h(static_cast<const uint8_t *>(d_src.p), w, h, t, t + OUT, t + 2 * OUT, ch.ksize, static_cast<uint8_t *>(d_tmp.p), OUT, s);
    launch_resample_v_norm(static_cast<const uint8_t *>(d_tmp.p), OUT, t + voff, t + voff + OUT, t + voff + 2 * OUT, cv.ksize, static_cast<float *>(d_out.p), OUT, mean, sd, s);
    HIP_CHECK(hipMemcpyAsync(out_chw, d_out.p, out_bytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

void Engine::release_buffers() {
    for (Conversation &c : conv_) { if (c.graph) HIP_IGNORE(hipGraphExecDestroy(c.graph)); c.graph = nullptr; }
    for (hipGraphExec_t &g : batch_graph_) { if (g) HIP_IGNORE(hipGraphExecDestroy(g)); g = nullptr; }
    spec_drop_graphs();
    if (h_argmax_) HIP_IGNORE(hipHostFree(h_argmax_));
    if (h_bstage_) HIP_IGNORE(hipHostFree(h_bstage_));
    if (h_logits_) HIP_IGNORE(hipHostFree(h_logits_));
    if (h_seg_) HIP_IGNORE(hipHostFree(h_seg_));
    h_argmax_ = nullptr; h_bstage_ = nullptr; h_logits_ = nullptr; h_seg_ = nullptr; logits_host_slot_ = -1;
    buf_arena_.release();
}
Engine::~Engine() {
    if (trace_file_) { fclose(trace_file_); trace_file_ = nullptr; }
    if (stream_hung_) {   // see engine.hpp: leak the device side, touch nothing that synchronises
        llm_arena_.abandon(); vis_arena_.abandon(); buf_arena_.abandon(); ri_arena_.abandon(); vgen_arena_.abandon();
        // the owning members would free themselves right after this body: hipFree / hipHostFree wait for a stream that never drains.  Every handle of the class is
        // listed here and nowhere else
        abandon_all(pfx_k_, pfx_v_, score_buf_, score_lp_, score_glp_, score_tgt_, score_greedy_, topn_d_, topn_h_, topn_in_, topn_hin_, topn_ev_,
                    pen_, spec_logits_, spec_res_, spec_hres_, beam_d_, beam_h_, beam_save_, beam_ev_,
                    guide_mix_, guide_d_, guide_h_, guide_ev_, con_vocab_, con_off_, con_stage_, con_row_h_,
                    state_d_[0], state_d_[1], state_h_[0], state_h_[1], state_sum_d_, state_sum_h_, state_cs_, state_ev_kernel_[0], state_ev_kernel_[1], state_ev_copy_[0],
                    state_ev_copy_[1], smp_, smpx_, sdr_res_, sdr_hres_);
        for (Constraint &c : con_) c.dev.abandon();
        return;
    }
    if (stream_) HIP_IGNORE(hipStreamSynchronize(stream_));
    for (auto &e : site_events_) { HIP_IGNORE(hipEventDestroy(e.a)); HIP_IGNORE(hipEventDestroy(e.b)); }
    if (stage_) HIP_IGNORE(hipFree(stage_));
    release_buffers();                                                       // (the features' own buffers free themselves behind this body: the stream has drained)
    if (stream_) HIP_IGNORE(hipStreamDestroy(stream_));
}
void Engine::sync() { (void)flush(); HIP_CHECK(hipStreamSynchronize(stream_)); }

// ====================================================================================================================
// init / load
// ====================================================================================================================
// The launch tuning of a context: the defaults, the device's CU count and the five environment switches that choose among launch forms.  Read per context, at load --
// a later context with the variable unset has the default again.
LaunchTuning launch_tuning_from_env(int cus) {
    LaunchTuning t;
    t.cus = cus;
    if (const char *e = getenv("MINIGPT4_ATTN_PREFILL_W8")) t.attn_prefill_w8 = atoi(e);   // 0: prompt attention without the 8-wave loader / MFMA form
    if (const char *e = getenv("MINIGPT4_MMQH")) t.mmqh = atoi(e);                         // 1: Q4_K / Q5_K prompt rows on the fp16-MFMA form with scaled operands (measured SLOWER; A/B)
    if (const char *e = getenv("MINIGPT4_ATTN_QT")) t.attn_vit_qt = atoi(e);               // query tiles per workgroup of the ViT / Q-Former attention (1 = the rounds 2-5 form; A/B, bit-identical)
    if (const char *e = getenv("MINIGPT4_SPLITK_XCD")) t.splitk_xcd = atoi(e);             // 0: split-K GEMM slices in grid.z, every XCD walks every slice (rounds 3-5; A/B, bit-identical)
    if (const char *e = getenv("MINIGPT4_F16_KS")) t.f16_ks = atoi(e);                     // forced K split of the F16 language model's single-matrix prompt launches (wo, w2; A/B)
    return t.normalised();
}
int Engine::init(const std::string &vision_path, const std::string &llm_path, int seed, int n_ctx, int n_batch) {
    const int ndev = device_count_noexcept();
    if (ndev <= 0) { set_last_error("no HIP device visible: the MI355X engine has no CPU fallback"); MG4_ERR("%s", last_error().c_str()); return E_LoadLanguageModel; }
    // native multi-GPU load (dist.hpp): MINIGPT4_WORLD_SIZE / MINIGPT4_RANK / MINIGPT4_NCCL_ID_FILE -> rank 0 reads the files, every other rank loads
    // headers only and receives both weight arenas by ncclBroadcast inside this call.  Parsed BEFORE the device is chosen: the stream, the arenas and
    // the communicator must all be created on the device the rank ends up on (round-5 advisor: the stream used to be created on device 0 first).
    DistEnv dist; { std::string derr; if (parse_dist_env(dist, derr)) { set_last_error(derr); MG4_ERR("%s", derr.c_str()); return E_LoadLanguageModel; } }
    const char *dv = getenv("MINIGPT4_DEVICE");
    if (!dv) dv = getenv("LOCAL_RANK");
    device_ = dv ? atoi(dv) % ndev : (dist.active() && dist.world > 1 ? dist.rank % ndev : 0);
    if (!dv && dist.active() && dist.world > 1) MG4_INFO("no MINIGPT4_DEVICE / LOCAL_RANK: rank %d takes device %d", dist.rank, device_);
    HIP_CHECK(hipSetDevice(device_));
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, device_));
    MG4_INFO("device %d: %s (%s), %d CUs, %.1f GiB", device_, prop.name, prop.gcnArchName, prop.multiProcessorCount, prop.totalGlobalMem / 1073741824.0);
    // The library is built for gfx950 only, and its in-launch hand-offs (K-split tickets of k_matvec_ri, the key-split attention's arrival counters) rely on that part's cache
    // behaviour -- write-through agent-scope stores + vmcnt(0) before the ticket, cache-bypassing agent-scope loads after it, no fences (MI355X_MICROARCH.md "Valid forms"): refuse
    // any other device by name instead of failing at the first launch (or, worse, not failing)
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_last_error(std::string("device ") + prop.gcnArchName + " is not gfx950 (MI355X): this library carries gfx950 code objects only"); MG4_ERR("%s", last_error().c_str());
        return E_LoadLanguageModel;
    }
    HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    n_ctx_ = n_ctx > 0 ? n_ctx : 2048;
    n_batch_ = n_batch > 0 ? n_batch : 512;
    max_rows_ = std::max(n_batch_, 32);
    // Run-time switches read here, once (no launcher calls getenv).  What is left after round 4's pruning: device / conversation count / load mode /
    // parity mode, the graph switch the profiling tools use, and the five arms the bit-identity tests compare against (tests/test_gpu_parity.py,
    // tests/test_gpu_batch.py).  Tile shapes, K splits and the other experiment parameters are reachable only through the test library's setters
    // (include/minigpt4_amd_test.h).
    use_graph_ = !(getenv("MINIGPT4_NO_GRAPH") && atoi(getenv("MINIGPT4_NO_GRAPH")));
    max_chunk_ = max_rows_;
    if (const char *dc = getenv("MINIGPT4_DEFER_COMBINE")) defer_combine_ = atoi(dc) != 0;                    // 0: every K-split combine as its own launch
    // bit mask: 1 w1|w3 + silu*mul in one launch, 4 the attention kernel stores fp16 rows for wo
    if (const char *fp = getenv("MINIGPT4_F16_PAIR")) f16_pair_ = atoi(fp);
    // 0: wq|wk and wv of a mixed-type layer as two launches (batched step)
    batch_mix_ = !(getenv("MINIGPT4_BATCH_MIX") && atoi(getenv("MINIGPT4_BATCH_MIX")) == 0);
    if (const char *e = getenv("MINIGPT4_ATTN_SPLIT_T")) attn_split_t_ = atoi(e);   // cached keys from which the decode step uses the key-split attention (0 = never)
    // workgroups per head of the one-row decode attention, each with its own share of the value columns (llm_kernels.hip: VS): 0 = choose (Engine::forward: 4 while
    // 4 x heads fit the CUs -- 376.2-376.4 against 370.5-371.0 tok/s at 40 heads, profiles/r12_decode_attention_vsplit.log), 1 / 2 / 4 = force
    if (const char *e = getenv("MINIGPT4_ATTN_VS")) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4) attn_vs_ = v; }
    if (const char *e = getenv("MINIGPT4_MV_IB")) { const int v = atoi(e); if (v == 0 || v == 1) for (bool &b : mv_issue_bar_) b = v != 0; }   // unset: the per-site defaults
    tune_ = launch_tuning_from_env(prop.multiProcessorCount);   // the CU count and the five launch switches (MINIGPT4_ATTN_PREFILL_W8, _MMQH, _ATTN_QT, _SPLITK_XCD, _F16_KS)
    // 0: the decode step gathers exp / SiLU from ggml's fp16 tables like rounds 1-4 (A/B)
    if (const char *e = getenv("MINIGPT4_COMPUTED_TABLES")) computed_tables_ = atoi(e) != 0;
    // 1: the MFMA batched launches norm + quantise their rows themselves (measured SLOWER: 864 vs 987 tok/s at B = 4; A/B)
    if (const char *e = getenv("MINIGPT4_RI_FUSE")) ri_fuse_ = atoi(e) != 0;
    // 0: w2 of the 4-conversation step on the v_dot4 launch instead of the K-split MFMA launch (A/B: profiles/r05_batched_decode_inengine.log)
    if (const char *e = getenv("MINIGPT4_RI_W2")) ri_w2_ = atoi(e) != 0;
    // 1: wo of the 3- / 4-conversation step on the MFMA launch with the plain quantisation of the attention rows inside it (round 6, A/B)
    if (const char *e = getenv("MINIGPT4_RI_WO")) ri_wo_ = atoi(e) != 0;
    // 0: batched decode on the v_dot4 multi-row mat-vec (rounds 2-4), no row-interleaved image
    if (const char *e = getenv("MINIGPT4_RI")) use_ri_ = atoi(e) != 0;
    // 0: the Q-Former's image-independent head is recomputed per encode (round-4 form, A/B)
    if (const char *e = getenv("MINIGPT4_QF_FOLD")) qf_fold_ = atoi(e) != 0;
    // K slices of the ViT's attention projection (1 = whole K + standalone LayerNorm: the default since round 3; 2..: split-K + the reduce that also normalises; A/B)
    if (const char *e = getenv("MINIGPT4_SPLITK_PROJ")) splitk_proj_ = std::max(1, std::min(SPLITK_MAX, atoi(e)));
    if (const char *e = getenv("MINIGPT4_SPLITK_FC2")) splitk_fc2_ = std::max(1, std::min(SPLITK_MAX, atoi(e)));     // K slices of the ViT's fc2 (default 4; A/B)
    // decode step: which row preparations ride in their consumer's prologue (bit 0 qkv, 1 wo, 2 w1|w3, 3 w2 <- SiLU * mul + quantisation, 4 output, 5 pair, 6 mixed qkv; default 87; A/B)
    if (const char *e = getenv("MINIGPT4_FUSE")) fuse_mask_ = atoi(e);
    if (const char *e = getenv("MINIGPT4_PAIR_SILU_COMPUTED")) pair_silu_computed_ = atoi(e) != 0;   // 0: the F16 model's w1 | w3 pair epilogue gathers SiLU from the fp16 table (A/B)
    if (const char *e = getenv("MINIGPT4_COMPUTED_GELU")) computed_gelu_ = atoi(e) != 0;   // 0: the vision GEMMs' GELU epilogues gather from the fp16 table (A/B)
    if (const char *e = getenv("MINIGPT4_QKV_HEAD_MAJOR")) qkv_head_major_ = atoi(e) != 0;
    if (const char *e = getenv("MINIGPT4_QF_SPLITK")) qf_splitk_ = atoi(e) != 0;     // 0: the Q-Former's dense / output layers as whole-K launches + standalone LayerNorm (A/B)
    if (const char *e = getenv("MINIGPT4_KV_HOIST")) kv_hoist_ = atoi(e) != 0;     // 0: one K | V projection GEMM per cross-attention layer (round-4 form, A/B)
    if (const char *ns = getenv("MINIGPT4_CONVERSATIONS")) conv_.assign((size_t)std::max(1, std::min(MAX_CONVERSATIONS, atoi(ns))), Conversation{});
    sampler_.seed(seed);
    smp_load_seed_ = (uint32_t)seed; smp_reseed();
    if (const char *tf = getenv("MINIGPT4_PARITY_TRACE")) { if (*tf) trace_file_ = fopen(tf, "wb"); }
    // oracle-order fp32 accumulation (forward_ref): bit-identical to the CPU oracle, slow
    parity_ = trace_file_ || (getenv("MINIGPT4_PARITY") && atoi(getenv("MINIGPT4_PARITY")));
    if (const char *e = getenv("MINIGPT4_STATE_BLOCK_BYTES")) { const long long v = atoll(e); if (v > 0) state_block_bytes_ = (size_t)v; }   // bytes of one snapshot block (default 32 MiB; tests force several blocks on tiny models)
    pen_mode_ = getenv("MINIGPT4_PENALTIES") && atoi(getenv("MINIGPT4_PENALTIES"));   // the reference's unmodified binding / web UI: its penalty arguments are honoured
    if (const char *lm = getenv("MINIGPT4_LOAD")) load_mode_ = !strcmp(lm, "recv") ? LOAD_RECV : LOAD_FULL;
    // the exchange decides who reads the files: MINIGPT4_LOAD=recv on rank 0 would broadcast empty arenas
    if (dist.active()) load_mode_ = dist.rank != 0 ? LOAD_RECV : LOAD_FULL;
    // With the native exchange active a load error on THIS rank is not returned at once: the rank still joins the communicator and reports it there,
    // so that its peers fail with it instead of waiting for it inside RCCL (native_broadcast).
    int load_err = E_None;
    auto t0 = std::chrono::steady_clock::now();
    try {
        load_err = load_llm(llm_path);
        auto t1 = std::chrono::steady_clock::now();
        if (!load_err) MG4_INFO("LLM model init took %lld ms to complete", (long long)std::chrono::duration_cast<std::chrono::milliseconds>(t1 - t0).count());
        if (!load_err) load_err = load_vision(vision_path);
        auto t2 = std::chrono::steady_clock::now();
        if (!load_err) MG4_INFO("Loading minigpt4 model took %lld ms to complete", (long long)std::chrono::duration_cast<std::chrono::milliseconds>(t2 - t1).count());
        // LOAD_RECV: weights_received() derives both.  MINIGPT4_CONVERSATIONS > 1 sizes the context like set_conversations(n) does, row-interleaved image included
        if (!load_err) { alloc_buffers(); if (load_mode_ == LOAD_FULL) { fold_qformer_constants(); if (conv_.size() > 1) build_ri_planes(); } }
    } catch (const HipError &e) {
        if (!dist.active()) throw;
        set_last_error(std::string("load failed: ") + e.what + " (" + hipGetErrorString(e.code) + ")"); load_err = E_LoadLanguageModel;
    }
    if (stage_) { HIP_IGNORE(hipFree(stage_)); stage_ = nullptr; stage_cap_ = 0; }
    if (dist.active()) { if (int e = native_broadcast(dist.world, dist.rank, dist.id_file, dist.timeout_s, load_err)) return load_err ? load_err : e; }
    return load_err;
}

// The load-time exchange of a node's replicas, inside the C library: unique id through a file, communicator, layout agreement, both arenas from rank
// 0 in <= 1 GiB pieces, checksum agreement.  Any failure is an error of minigpt4_model_load (message in minigpt4_amd_last_error); there is no
// fallback to reading the files.
int Engine::native_broadcast(int world, int rank, const std::string &id_file, int timeout_s, int local_err) {
    std::string err;
    // round 5 (advisor): EVERY rank takes part in the same sequence of collectives and learns the same verdict, so a failure anywhere fails the load
    // everywhere instead of leaving the healthy ranks inside a collective for ever: (1) a rank whose own load failed (header error, unsupported
    // tensor) still joins and says so; (2) agreement is a symmetric all-reduce (element-wise max of {x, ~x} = max and min of every word, plus an "I
    // am fine" flag), not a one-way broadcast only the receivers compare; (3) ncclCommInitRank runs under a watchdog (dist.cpp) and the stream waits
    // below are bounded by MINIGPT4_DIST_TIMEOUT_S.
    auto fail = [&](const std::string &what) {
        if (rank == 0) unlink(id_file.c_str());        // never leave an id behind that a later job could pick up
        set_last_error("weight broadcast (rank " + std::to_string(rank) + " of " + std::to_string(world) + "): " + what); MG4_ERR("%s", last_error().c_str()); return (int)E_LoadLanguageModel; };
    // the Rccl object outlives a timed-out bootstrap on purpose (its helper thread is still inside the library): heap-allocated, leaked when poisoned
    struct Holder { Rccl *r = new Rccl; ~Holder() { if (r && !r->poisoned()) delete r; } } holder;
    Rccl &rccl = *holder.r;
    if (rccl.open(err)) return fail(err);
    uint8_t id[128];
    if (rank == 0) { unlink(id_file.c_str()); if (rccl.unique_id(id, err) || publish_unique_id(id_file, id, err)) return fail(err); }
    else if (await_unique_id(id_file, id, timeout_s, err, process_start_epoch_s())) return fail(err);
    if (rccl.init(world, rank, id, timeout_s, err)) return fail(err);
    if (rank == 0) unlink(id_file.c_str());            // every rank has joined: a later job must not pick this id up
    const auto t0 = std::chrono::steady_clock::now();
    auto wait_stream = [&](const char *what) -> bool {   // bounded hipStreamSynchronize: a peer that died inside a collective must not hang this rank
        const auto w0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t q = hipStreamQuery(stream_);
            if (q == hipSuccess) return true;
            if (q != hipErrorNotReady) { (void)hipGetLastError(); err = std::string(what) + ": " + hipGetErrorString(q); return false; }
            if (std::chrono::steady_clock::now() - w0 > std::chrono::seconds(timeout_s)) {
                // the collective (and the copies queued behind it) are STILL on the stream: nothing they touch may be freed, and the communicator must not be
                // destroyed under them -- poison the Rccl object (communicator and library leaked), leak the word buffers (Words below), fail the load
                rccl.poison(); stream_hung_ = true;
                err = std::string(what) + " did not complete within " + std::to_string(timeout_s) + " s (a peer left the exchange?)"; return false;
            }
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
    };
    // device words of the agreements + a PINNED host image of them (the device-to-host copy behind a hung collective may land long after this frame is gone: never a
    // stack array).  Both are leaked when the exchange was poisoned: hipFree would synchronise with the hung stream.
    struct Words { Rccl &r; unsigned long long *d = nullptr, *h = nullptr; ~Words() { if (r.poisoned()) return; if (d) HIP_IGNORE(hipFree(d)); if (h) HIP_IGNORE(hipHostFree(h)); } } words{rccl};
    HIP_CHECK(hipMalloc((void **)&words.d, 128));
    HIP_CHECK(hipHostMalloc((void **)&words.h, 256, hipHostMallocDefault));
    unsigned long long *const d_words = words.d;
    // Symmetric agreement: true on EVERY rank iff every rank passed ok and all ranks hold the same four words; otherwise false on every rank, with a
    // message naming the cause.
    auto agree = [&](const unsigned long long mine[4], bool ok_here, const char *what) -> bool {
        unsigned long long *const v = words.h, *const r = words.h + 16;
        for (int i = 0; i < 4; i++) { v[i] = mine[i]; v[4 + i] = ~mine[i]; }
        v[8] = ok_here ? 0ull : 1ull;                    // max over ranks: 1 = somebody failed before this point
        v[9] = ok_here ? 0ull : (unsigned long long)(rank + 1);   // ... and (one of) who
        HIP_CHECK(hipMemcpyAsync(d_words, v, 80, hipMemcpyHostToDevice, stream_));
        if (rccl.allreduce_max_u64(d_words, 10, stream_, err)) return false;
        HIP_CHECK(hipMemcpyAsync(r, d_words, 80, hipMemcpyDeviceToHost, stream_));
        if (!wait_stream(what)) return false;
        if (r[8]) { err = std::string("rank ") + std::to_string((long long)r[9] - 1) + " failed before \"" + what + "\"" + (ok_here ? "" : " (this rank: " + last_error() + ")"); return false; }
        for (int i = 0; i < 4; i++) if (r[i] != ~r[4 + i]) {   // max != min: the ranks disagree
            char b[256]; snprintf(b, sizeof b, "%s differ between the ranks (word %d: max %llx, min %llx; this rank %llx)", what, i, r[i], ~r[4 + i], mine[i]); err = b; return false; }
        return true;
    };
    // test injection (tests/test_gpu_serve.py::test_native_broadcast_stream_timeout_leaks_and_returns): a bounded busy kernel in front of the first collective stands in
    // for a collective whose peer died -- the bounded wait below must give up, poison the exchange and return without touching the stream again
    if (const char *st = getenv("MINIGPT4_DIST_TEST_STALL_MS")) launch_stall((unsigned)std::max(0, atoi(st)), stream_);
    const ArenaPlan pl = arena_plan();
    const unsigned long long plan_words[4] = {(unsigned long long)pl.llm_bytes, (unsigned long long)pl.vision_bytes, (unsigned long long)pl.llm_hash, (unsigned long long)pl.vision_hash};
    if (!agree(plan_words, local_err == 0, "arena layouts (sizes / layout hashes)")) return fail(err);
    if (rccl.broadcast(llm_arena_.base, llm_arena_.used, 0, stream_, err) || rccl.broadcast(vis_arena_.base, vis_arena_.used, 0, stream_, err)) return fail(err);
    if (!wait_stream("the arena broadcast")) return fail(err);
    dist_bcast_ms_ = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    bool derived_ok = true;
    try { if (load_mode_ == LOAD_RECV) weights_received(); } catch (const HipError &e) { derived_ok = false; set_last_error(std::string("weights_received: ") + e.what); }
    unsigned long long sums[4] = {0ull, 0ull, 0ull, 0ull};
    if (derived_ok) { sums[0] = device_checksum(llm_arena_.base, llm_arena_.used, stream_); sums[1] = device_checksum(vis_arena_.base, vis_arena_.used, stream_); }
    if (!agree(sums, derived_ok, "arena contents (checksums) after the broadcast")) return fail(err);
    dist_world_ = world; dist_rank_ = rank;
    MG4_INFO("rank %d of %d: weight arenas %s in %.1f ms (%.2f GB, RCCL)", rank, world, rank ? "received" : "broadcast", dist_bcast_ms_, (llm_arena_.used + vis_arena_.used) / 1e9);
    return E_None;
}

// LOAD_RECV: the two weight arenas have been filled from rank 0 (broadcast): everything derived from them on the device
int Engine::weights_received() {
    if (load_mode_ != LOAD_RECV) return 0;
    load_mode_ = LOAD_FULL;
    const size_t NQ = (size_t)v_nq_;
    for (size_t b = 0; b < (size_t)VISION_BATCH_MAX; b++) HIP_CHECK(hipMemcpy(vi_qtok_rep_ + b * NQ * 768, v_qtok_, NQ * 768 * 4, hipMemcpyDeviceToDevice));
    fold_qformer_constants();
    if (conv_.size() > 1) build_ri_planes();               // set_conversations(n > 1) ran while the arenas were still empty
    return 0;
}
// Host only: the arena layout (sizes + layout hashes) the two files produce, without a device: what a receiving rank must reproduce
// (tests/test_cpu_dist.py).
int Engine::plan_arenas(const std::string &vision_path, const std::string &llm_path, ArenaPlan &out) {
    Engine e;
    e.load_mode_ = LOAD_PLAN;
    e.llm_arena_.virt = e.vis_arena_.virt = true;
    if (int err = e.load_llm(llm_path)) return err;
    if (int err = e.load_vision(vision_path)) return err;
    out = e.arena_plan();
    return 0;
}

// Tensor types the kernels do not stream natively but that have an exact image in one they do: Q3_K -> Q6_K (quantize.hpp).  The conversion runs on
// the host at load.
static int effective_type(int t) { return t == GT_Q3_K ? GT_Q6_K : t; }
static bool tensor_type_loadable(int t) { return qweight_supported(effective_type(t)); }
// bytes of a tensor as the GPU holds it
static size_t effective_nbytes(const TensorMeta &t) { return t.type == GT_Q3_K ? t.nbytes / 110 * 210 : t.nbytes; }

void Engine::upload_qweight(const TensorMeta &t0, const uint8_t *file_base0, QWeight &w) {
    TensorMeta t = t0;
    const uint8_t *file_base = file_base0;
    std::vector<uint8_t> conv;
    if (t0.type == GT_Q3_K) {
        conv.resize(moves_data() ? effective_nbytes(t0) : 0);
        if (moves_data()) q3k_to_q6k(file_base0 + t0.offset, conv.data(), t0.nbytes / 110);
        t.type = GT_Q6_K; t.nbytes = effective_nbytes(t0); t.offset = 0; file_base = conv.data();
    }
    const int cols = (int)t.ne[0], rows = (int)t.ne[1];
    QWeight plan;
    const size_t need = plan_qweight(t.type, rows, cols, plan, nullptr);
    uint8_t *base = llm_arena_.take(need);
    plan_qweight(t.type, rows, cols, w, base);
    if (!moves_data()) return;                                              // LOAD_RECV / LOAD_PLAN: layout only
    if (t.type == GT_F16 || t.type == GT_F32) { HIP_CHECK(hipMemcpy(base, file_base + t.offset, t.nbytes, hipMemcpyHostToDevice)); return; }
    if (t.nbytes > stage_cap_) throw HipError{hipErrorOutOfMemory, "staging buffer too small", __FILE__, __LINE__};
    HIP_CHECK(hipMemcpy(stage_, file_base + t.offset, t.nbytes, hipMemcpyHostToDevice));
    launch_repack(stage_, w, stream_);
    HIP_CHECK(hipStreamSynchronize(stream_));
}

int Engine::load_llm(const std::string &path) {
    if (int e = llm_.load(path)) { MG4_ERR("failed to parse %s: %s", path.c_str(), last_error().c_str()); return e; }
    tok_.init(llm_);
    const int E = (int)llm_.n_embd, L = (int)llm_.n_layer, V = (int)llm_.n_vocab, F = (int)llm_.n_ff();
    const int hd = E / (int)llm_.n_head;
    if (!attn_head_size_supported(hd)) { set_last_error("unsupported head size (supported: 32, 64, 128)"); return E_LoadLanguageModel; }
    // k_attn_llm keeps one fp32 score + one fp16 probability per key of the context in LDS (6 bytes per key, 160 KiB per workgroup): refuse what
    // cannot launch
    if (parity_) attn_ref_prepare();
    auto ctx_too_long = [&](const char *which, int lim) {
        set_last_error(std::string(which) + "n_ctx " + std::to_string(n_ctx_) + " exceeds what the attention kernel's LDS score rows hold (" + std::to_string(lim) + ")");
        MG4_ERR("%s", last_error().c_str());
        return (int)E_LoadLanguageModel;
    };
    if (parity_ && n_ctx_ > attn_ref_max_ctx(hd)) return ctx_too_long("MINIGPT4_PARITY (oracle-order kernel): ", attn_ref_max_ctx(hd));
    if (n_ctx_ > attn_max_ctx(hd)) return ctx_too_long("", attn_max_ctx(hd));
    MG4_INFO("llm: n_vocab %d n_embd %d n_head %u n_layer %d n_ff %d n_ctx %d", V, E, llm_.n_head, L, F, n_ctx_);
    auto need = [&](const std::string &name, int64_t ne0, int64_t ne1) -> const TensorMeta * {
        const TensorMeta *t = llm_.find(name);
        if (!t) { set_last_error("LLM file: missing tensor " + name); return nullptr; }
        if (t->ne[0] != ne0 || (ne1 ? (t->ne.size() != 2 || t->ne[1] != ne1) : t->ne.size() != 1)) { set_last_error("LLM file: bad shape for " + name); return nullptr; }
        if (ne1 == 0 && t->type != GT_F32) { set_last_error("LLM file: " + name + " must be f32"); return nullptr; }
        if (ne1 && !tensor_type_loadable(t->type)) { set_last_error(std::string("LLM file: tensor type ") + gt_name(t->type) + " of " + name + " is not supported by the gfx950 kernels"); return nullptr; }
        return t;
    };
    // pass 1: validate + size the arena
    size_t total = 0, max_raw = 0;
    QWeight tmp;
    std::vector<std::pair<std::string, std::pair<int64_t, int64_t>>> mats;
    mats.push_back({"output.weight", {E, V}});
    for (int i = 0; i < L; i++) {
        const std::string p = "layers." + std::to_string(i) + ".";
        for (const char *w : {"attention.wq.weight", "attention.wk.weight", "attention.wv.weight", "attention.wo.weight"}) mats.push_back({p + w, {E, E}});
        mats.push_back({p + "feed_forward.w1.weight", {E, F}});
        mats.push_back({p + "feed_forward.w2.weight", {F, E}});
        mats.push_back({p + "feed_forward.w3.weight", {E, F}});
    }
    wbytes_token_ = 0;
    for (auto &m : mats) {
        const TensorMeta *t = need(m.first, m.second.first, m.second.second);
        if (!t) { MG4_ERR("%s", last_error().c_str()); return E_LoadLanguageModel; }
        total += plan_qweight(effective_type(t->type), (int)t->ne[1], (int)t->ne[0], tmp, nullptr) + 256;
        if (t->type != GT_F16 && t->type != GT_F32) max_raw = std::max(max_raw, effective_nbytes(*t));
        wbytes_token_ += effective_nbytes(*t);                             // what a decoded token streams from HBM
    }
    const TensorMeta *tt = llm_.find("tok_embeddings.weight");
    if (!tt || tt->ne.size() != 2 || tt->ne[0] != E || tt->ne[1] != V || !tensor_type_loadable(tt->type)) { set_last_error("LLM file: bad tok_embeddings.weight"); MG4_ERR("%s", last_error().c_str()); return E_LoadLanguageModel; }
    total += effective_nbytes(*tt) + 256;
    wbytes_token_ += gt_nbytes(effective_type(tt->type), (size_t)E);
    for (int i = 0; i < L; i++) for (const char *n : {"attention_norm.weight", "ffn_norm.weight"}) if (!need("layers." + std::to_string(i) + "." + n, E, 0)) { MG4_ERR("%s", last_error().c_str()); return E_LoadLanguageModel; }
    if (!need("norm.weight", E, 0)) { MG4_ERR("%s", last_error().c_str()); return E_LoadLanguageModel; }
    total += (size_t)(2 * L + 1) * ((size_t)E * 4 + 256);
    wbytes_token_ += (size_t)(2 * L + 1) * E * 4;
    llm_arena_.alloc(total + 4096);
    if (max_raw && moves_data()) { HIP_CHECK(hipMalloc((void **)&stage_, max_raw)); stage_cap_ = max_raw; }
    // pass 2: upload + repack
    const uint8_t *fb = llm_.mf.data;
    upload_qweight(*llm_.find("output.weight"), fb, output_);
    layers_.resize((size_t)L);
    for (int i = 0; i < L; i++) {
        const std::string p = "layers." + std::to_string(i) + ".";
        LayerW &lw = layers_[(size_t)i];
        upload_qweight(*llm_.find(p + "attention.wq.weight"), fb, lw.wq);
        upload_qweight(*llm_.find(p + "attention.wk.weight"), fb, lw.wk);
        upload_qweight(*llm_.find(p + "attention.wv.weight"), fb, lw.wv);
        upload_qweight(*llm_.find(p + "attention.wo.weight"), fb, lw.wo);
        upload_qweight(*llm_.find(p + "feed_forward.w1.weight"), fb, lw.w1);
        upload_qweight(*llm_.find(p + "feed_forward.w2.weight"), fb, lw.w2);
        upload_qweight(*llm_.find(p + "feed_forward.w3.weight"), fb, lw.w3);
        const TensorMeta *an = llm_.find(p + "attention_norm.weight"), *fn = llm_.find(p + "ffn_norm.weight");
        lw.attn_norm = upload_raw<float>(llm_arena_, fb + an->offset, an->nbytes);
        lw.ffn_norm = upload_raw<float>(llm_arena_, fb + fn->offset, fn->nbytes);
    }
    const TensorMeta *nt = llm_.find("norm.weight");
    norm_ = upload_raw<float>(llm_arena_, fb + nt->offset, nt->nbytes);
    if (tt->type == GT_Q3_K) {   // the embedding gather dequantises raw ggml rows: give it the (value-identical) Q6_K rows
        std::vector<uint8_t> conv(moves_data() ? effective_nbytes(*tt) : 0);
        if (moves_data()) q3k_to_q6k(fb + tt->offset, conv.data(), tt->nbytes / 110);
        tok_raw_ = upload_raw<uint8_t>(llm_arena_, conv.data(), effective_nbytes(*tt));
    } else tok_raw_ = upload_raw<uint8_t>(llm_arena_, fb + tt->offset, tt->nbytes);
    tok_type_ = effective_type(tt->type);
    MG4_INFO("llm weights: %.1f MB in HBM, %.3f GB streamed per decoded token", llm_arena_.used / 1048576.0, wbytes_token_ / 1e9);
    return E_None;
}

int Engine::load_vision(const std::string &path) {
    if (int e = vis_.load(path)) { MG4_ERR("failed to parse %s (%s)", path.c_str(), last_error().c_str()); return e; }
    auto fail = [&](const std::string &msg, int code) { set_last_error("vision file: " + msg); MG4_ERR("%s", last_error().c_str()); return code; };
    const TensorMeta *pos = vis_.find("visual_encoder", "pos_embed");
    if (!pos || pos->ne.size() != 2 || pos->type != GT_F32) return fail("missing/bad visual_encoder.pos_embed", E_LoadModelFileHeader);
    v_D_ = (int)pos->ne[0];
    if (pos->ne[1] != 257 || v_D_ % 88 || v_D_ % 16) return fail("pos_embed must be [D,257] with D a multiple of 88 and 16 (head size 88 is hard-coded in the reference, minigpt4.cpp:1271)", E_LoadModelFileHeader);
    v_heads_ = v_D_ / 88;
    if (vis_.config_int("encoder_width", v_D_) != v_D_) return fail("config Qformer.encoder_width disagrees with pos_embed", E_LoadModelFileHeader);
    v_depth_ = 0;
    while (vis_.find("visual_encoder", "blocks." + std::to_string(v_depth_) + ".norm1.weight")) v_depth_++;
    if (!v_depth_) return fail("no ViT blocks", E_LoadModelFileHeader);
    const TensorMeta *fc1 = vis_.find("visual_encoder", "blocks.0.mlp.fc1.weight");
    if (!fc1 || fc1->ne.size() != 2) return fail("missing blocks.0.mlp.fc1.weight", E_LoadModelFileHeader);
    v_M_ = (int)fc1->ne[1];
    const TensorMeta *qt = vis_.find("query_tokens", "weight");
    if (!qt || qt->ne.size() != 2 || qt->ne[0] != 768 || qt->type != GT_F32) return fail("bad query_tokens.weight", E_LoadModelFileHeader);
    v_nq_ = (int)qt->ne[1];
    // reference PANICs (minigpt4.cpp:2230)
    if (vis_.config_int("query_length", v_nq_) != v_nq_) return fail("query_embeds_length != query_length", E_LoadModelFileHeader);
    {   // sizes read from an untrusted header feed container sizes below
        const long long ql = vis_.config_int("num_hidden_layers", 12);
        if (ql < 1 || ql > 64 || v_nq_ < 1 || v_nq_ > 256) return fail("num_hidden_layers / query_length out of range", E_LoadModelFileHeader);
        v_ql_ = (int)ql;
    }
    const TensorMeta *lp = vis_.find("llama_proj", "weight");
    if (!lp || lp->ne.size() != 2 || lp->ne[0] != 768) return fail("bad llama_proj.weight", E_LoadModelFileHeader);
    v_out_ = (int)lp->ne[1];
    const TensorMeta *iq = vis_.find("Qformer", "bert.encoder.layer.0.intermediate_query.dense.weight");
    if (!iq || iq->ne.size() != 2) return fail("missing intermediate_query", E_LoadModelFileHeader);
    v_qi_ = (int)iq->ne[1];
    if (v_M_ % 16 || v_qi_ % 16) return fail("MLP widths must be multiples of 16", E_LoadModelFileHeader);

    // Linear weights: all F16 (the reference's published f16 files) -> the MFMA f16 GEMM path below; anything else -> the generic path
    // (engine_vision_generic.cpp)
    v_generic_ = false;
    for (auto &m : vis_.models) for (auto &t : m.second) {
        const TensorMeta &tm = t.second;
        const bool is_lin = tm.ne.size() == 2 && tm.name.size() >= 6 && tm.name.compare(tm.name.size() - 6, 6, "weight") == 0 && m.first != "query_tokens" && tm.name != "pos_embed" &&
                            tm.name.find("orm") == std::string::npos && tm.name != "patch_embed.proj.weight" && tm.name.find("embeddings") == std::string::npos;
        if (is_lin && tm.type != GT_F16) v_generic_ = true;
    }
    size_t total = 0;
    for (auto &m : vis_.models) for (auto &t : m.second) total += effective_nbytes(t.second) + 512 + (v_generic_ ? 2048 : 0);
    total += (size_t)v_D_ * 592 * 2 + (size_t)v_depth_ * 3 * v_D_ * 4 + (1 << 20);
    vis_arena_.alloc(total);
    const uint8_t *fb = vis_.mf.data;
    bool ok = true; std::string bad;
    auto f32v = [&](const std::string &model, const std::string &name, int64_t n) -> float * {
        const TensorMeta *t = vis_.find(model, name);
        if (!t || t->type != GT_F32 || t->nelements() != n) { ok = false; bad = model + "." + name; return nullptr; }
        return upload_raw<float>(vis_arena_, fb + t->offset, t->nbytes);
    };
    auto f16m = [&](const std::string &model, const std::string &name, int64_t n_in, int64_t n_out) -> const TensorMeta * {
        const TensorMeta *t = vis_.find(model, name);
        if (!t || t->ne.size() < 2 || t->nelements() != n_in * n_out) { ok = false; bad = model + "." + name; return nullptr; }
        if (t->type != GT_F16 && !v_generic_) { ok = false; bad = model + "." + name + " (unexpected type " + gt_name(t->type) + ")"; return nullptr; }
        return t;
    };
    // generic mode: the Linear weights are uploaded as QWeights by load_vision_generic(); the fp16 pointers of this path stay null
    auto up16 = [&](const TensorMeta *t) -> __half * { return t && !v_generic_ ? upload_raw<__half>(vis_arena_, fb + t->offset, t->nbytes) : nullptr; };
    auto concat16 = [&](const std::vector<const TensorMeta *> &ts) -> __half * {
        if (v_generic_) return nullptr;
        size_t bytes = 0; for (auto t : ts) { if (!t) return nullptr; bytes += t->nbytes; }
        uint8_t *d = vis_arena_.take(bytes); size_t off = 0;
        for (auto t : ts) { if (moves_data()) HIP_CHECK(hipMemcpy(d + off, fb + t->offset, t->nbytes, hipMemcpyHostToDevice)); off += t->nbytes; }
        return reinterpret_cast<__half *>(d);
    };
    auto concat32 = [&](const std::vector<std::pair<const char *, std::string>> &names, int64_t each) -> float * {
        uint8_t *d = vis_arena_.take((size_t)each * 4 * names.size()); size_t off = 0;
        for (auto &nm : names) { const TensorMeta *t = vis_.find(nm.first, nm.second);
            if (!t || t->type != GT_F32 || t->nelements() != each) { ok = false; bad = nm.second; return nullptr; }
            if (moves_data()) HIP_CHECK(hipMemcpy(d + off, fb + t->offset, t->nbytes, hipMemcpyHostToDevice)); off += t->nbytes; }
        return reinterpret_cast<float *>(d);
    };
    const int D = v_D_, M = v_M_;
    const char *VE = "visual_encoder";
    v_cls_ = f32v(VE, "cls_token", D);
    v_pos_ = f32v(VE, "pos_embed", (int64_t)D * 257);
    v_patch_b_ = f32v(VE, "patch_embed.proj.bias", D);
    const TensorMeta *pw = f16m(VE, "patch_embed.proj.weight", 588, D);
    if (pw && pw->type != GT_F16) { ok = false; bad = "visual_encoder.patch_embed.proj.weight (the conv kernel is always F16: convert.py:113-117, and minigpt4_quantize_model skips it)"; pw = nullptr; }
    if (pw) {   // [D][588] -> zero-padded [D][592] (MFMA K multiple of 16)
        std::vector<uint16_t> padded((size_t)D * 592, 0);
        const uint16_t *src = reinterpret_cast<const uint16_t *>(fb + pw->offset);
        for (int r = 0; r < D; r++) memcpy(&padded[(size_t)r * 592], src + (size_t)r * 588, 588 * 2);
        v_patch_w_ = upload_raw<__half>(vis_arena_, padded.data(), padded.size() * 2);
    }
    vblocks_.resize((size_t)v_depth_);
    for (int i = 0; i < v_depth_ && ok; i++) {
        const std::string p = "blocks." + std::to_string(i) + ".";
        VBlock &b = vblocks_[(size_t)i];
        b.n1w = f32v(VE, p + "norm1.weight", D); b.n1b = f32v(VE, p + "norm1.bias", D);
        b.n2w = f32v(VE, p + "norm2.weight", D); b.n2b = f32v(VE, p + "norm2.bias", D);
        // qkv bias = [q_bias, 0, v_bias] (minigpt4.cpp:1259-1262)
        const TensorMeta *qb = vis_.find(VE, p + "attn.q_bias"), *vb = vis_.find(VE, p + "attn.v_bias");
        if (!qb || !vb || qb->type != GT_F32 || vb->type != GT_F32 || qb->nelements() != D || vb->nelements() != D) { ok = false; bad = p + "attn.q_bias/v_bias"; break; }
        std::vector<float> bias3((size_t)3 * D, 0.0f);
        const float *qsrc = reinterpret_cast<const float *>(fb + qb->offset), *vsrc = reinterpret_cast<const float *>(fb + vb->offset);
        for (int j = 0; j < D; j++) { bias3[(size_t)j] = 0.0f + qsrc[j]; bias3[(size_t)2 * D + j] = 0.0f + vsrc[j]; }
        b.qkv_b = upload_raw<float>(vis_arena_, bias3.data(), bias3.size() * 4);
        b.qkv_w = up16(f16m(VE, p + "attn.qkv.weight", D, 3 * (int64_t)D));
        b.proj_w = up16(f16m(VE, p + "attn.proj.weight", D, D)); b.proj_b = f32v(VE, p + "attn.proj.bias", D);
        b.fc1_w = up16(f16m(VE, p + "mlp.fc1.weight", D, M)); b.fc1_b = f32v(VE, p + "mlp.fc1.bias", M);
        b.fc2_w = up16(f16m(VE, p + "mlp.fc2.weight", M, D)); b.fc2_b = f32v(VE, p + "mlp.fc2.bias", D);
    }
    v_lnv_w_ = f32v("ln_vision", "weight", D); v_lnv_b_ = f32v("ln_vision", "bias", D);
    v_qtok_ = f32v("query_tokens", "weight", (int64_t)768 * v_nq_);
    const char *QF = "Qformer";
    v_qeln_w_ = f32v(QF, "bert.embeddings.LayerNorm.weight", 768); v_qeln_b_ = f32v(QF, "bert.embeddings.LayerNorm.bias", 768);
    qlayers_.resize((size_t)v_ql_);
    // the K | V projections of every cross-attention layer as ONE contiguous block [n_cross * 1536][D] (+ biases): one GEMM per image batch instead
    // of one per cross layer
    {
        std::vector<const TensorMeta *> kvw; std::vector<std::pair<const char *, std::string>> kvb;
        v_ncross_ = 0;
        for (int i = 0; i < v_ql_; i++) {
            const std::string a = "bert.encoder.layer." + std::to_string(i) + ".crossattention.";
            if (!vis_.find(QF, a + "self.query.weight")) continue;
            kvw.push_back(f16m(QF, a + "self.key.weight", D, 768)); kvw.push_back(f16m(QF, a + "self.value.weight", D, 768));
            kvb.push_back({QF, a + "self.key.bias"}); kvb.push_back({QF, a + "self.value.bias"});
            qlayers_[(size_t)i].cross_idx = v_ncross_++;
        }
        if (v_ncross_ && ok) { v_kv_all_w_ = concat16(kvw); v_kv_all_b_ = concat32(kvb, 768); }
    }
    for (int i = 0; i < v_ql_ && ok; i++) {
        const std::string p = "bert.encoder.layer." + std::to_string(i) + ".";
        QLayer &L = qlayers_[(size_t)i];
        {   // self attention: Q,K,V share their input -> one [2304][768] GEMM
            const std::string a = p + "attention.";
            L.self.q_w = concat16({f16m(QF, a + "self.query.weight", 768, 768), f16m(QF, a + "self.key.weight", 768, 768), f16m(QF, a + "self.value.weight", 768, 768)});
            L.self.q_b = concat32({{QF, a + "self.query.bias"}, {QF, a + "self.key.bias"}, {QF, a + "self.value.bias"}}, 768);
            L.self.dense_w = up16(f16m(QF, a + "output.dense.weight", 768, 768)); L.self.dense_b = f32v(QF, a + "output.dense.bias", 768);
            L.self.ln_w = f32v(QF, a + "output.LayerNorm.weight", 768); L.self.ln_b = f32v(QF, a + "output.LayerNorm.bias", 768);
        }
        L.has_cross = vis_.find(QF, p + "crossattention.self.query.weight") != nullptr;   // detected by name (minigpt4.cpp:2008)
        if (L.has_cross) {
            const std::string a = p + "crossattention.";
            L.cross.q_w = up16(f16m(QF, a + "self.query.weight", 768, 768)); L.cross.q_b = f32v(QF, a + "self.query.bias", 768);
            L.cross.kv_w = v_kv_all_w_ ? v_kv_all_w_ + (size_t)L.cross_idx * 1536 * D : nullptr;          // this layer's [1536][D] slice of the shared block
            L.cross.kv_b = v_kv_all_b_ ? v_kv_all_b_ + (size_t)L.cross_idx * 1536 : nullptr;
            L.cross.dense_w = up16(f16m(QF, a + "output.dense.weight", 768, 768)); L.cross.dense_b = f32v(QF, a + "output.dense.bias", 768);
            L.cross.ln_w = f32v(QF, a + "output.LayerNorm.weight", 768); L.cross.ln_b = f32v(QF, a + "output.LayerNorm.bias", 768);
        }
        L.inter_w = up16(f16m(QF, p + "intermediate_query.dense.weight", 768, v_qi_)); L.inter_b = f32v(QF, p + "intermediate_query.dense.bias", v_qi_);
        L.out_w = up16(f16m(QF, p + "output_query.dense.weight", v_qi_, 768)); L.out_b = f32v(QF, p + "output_query.dense.bias", 768);
        L.oln_w = f32v(QF, p + "output_query.LayerNorm.weight", 768); L.oln_b = f32v(QF, p + "output_query.LayerNorm.bias", 768);
    }
    v_proj_w_ = up16(f16m("llama_proj", "weight", 768, v_out_)); v_proj_b_ = f32v("llama_proj", "bias", v_out_);
    if (!ok) return fail("missing or unsupported tensor " + bad, E_LoadModelFileHeader);
    if (v_generic_) {
        if (load_mode_ != LOAD_FULL) return fail("quantised / f32 vision files keep a third arena that the multi-GPU receive path does not cover: load them with LOAD_FULL on every rank", E_LoadModelFileHeader);
        if (int e = load_vision_generic()) return e;
    }
    MG4_INFO("vision weights: %.1f MB in HBM (ViT dim %d x %d blocks, Q-Former %d layers, proj -> %d)", vis_arena_.used / 1048576.0, v_D_, v_depth_, v_ql_, v_out_);
    return E_None;
}

void Engine::alloc_buffers() {
    const size_t S = conv_.size();
    max_rows_ = std::max(std::max(n_batch_, 32), (int)S);
    const size_t E = llm_.n_embd, F = llm_.n_ff(), V = llm_.n_vocab, L = llm_.n_layer, B = (size_t)max_rows_, C = (size_t)n_ctx_;
    const size_t Kmax = std::max(E, F), hd = E / llm_.n_head;
    const size_t D = (size_t)v_D_, M = (size_t)v_M_, NQ = (size_t)v_nq_;
    size_t total = 0;
    auto sz = [&](size_t b) { total += (b + 255) / 256 * 256 + 256; };
    sz(S * L * C * E * 2); sz(S * L * C * E * 2); sz(2 * C * (hd / 2) * 4 * 2); sz(3 * 65536 * 2);
    sz(5 * B * E * 4); sz(2 * B * F * 4); sz(S * V * 4); sz(S * V * 4); sz(8 * 256 + 2 * B * 4);
    sz(2 * B * Kmax); sz(B * Kmax / 256 * 4 + 64); sz(B * Kmax / 16 * 2 + 64); sz(B * Kmax / 16 + 64); sz(B * Kmax * 2); sz(B * Kmax / 8 + 128); sz(4 * (B * Kmax / 32 * 4 + 64)); sz(B * Kmax * 2); sz(B * Kmax * 4);
    sz(8192); sz((size_t)64 << 20); sz(attn_split_workspace_bytes((int)llm_.n_head, (int)hd, n_ctx_, std::max(attn_splits_forced_, attn_split_count((int)llm_.n_head, tune_.cus))));
    const size_t VB = (size_t)VISION_BATCH_MAX;                            // images encoded in one pass (minigpt4_amd_encode_images)
    sz(VB * 3 * 224 * 224 * 4); sz(VB * 256 * 592 * 2); sz(VB * 256 * D * 4); sz(VB * 257 * D * 4); sz(VB * 257 * 3 * D * 4); sz(VB * 3 * 257 * D * 2); sz(VB * 257 * M * 2);
    sz(VB * (size_t)SPLITK_MAX * 257 * D * 4);
    sz(VB * 9 * NQ * 2304 * 4); sz(VB * 257 * 1536 * 4 * (size_t)std::max(1, v_ncross_)); sz(VB * NQ * 768 * 4); sz(VB * NQ * 768 * 4); sz(VB * NQ * 768 * 2);
    sz(VB * NQ * (size_t)std::max(v_qi_, 768) * 2 * 4); sz(VB * NQ * (size_t)v_out_ * 4); sz(1 << 20);
    sz(seg_ints() * 4);
    buf_arena_.alloc(total);
    auto takef = [&](size_t n) { return reinterpret_cast<float *>(buf_arena_.take(n * 4)); };
    auto takeh = [&](size_t n) { return reinterpret_cast<__half *>(buf_arena_.take(n * 2)); };
    kc_ = takeh(S * L * C * E); vc_ = takeh(S * L * C * E);                // [conversation][layer][n_ctx][n_embd]
    HIP_CHECK(hipMemset(kc_, 0, S * L * C * E * 2)); HIP_CHECK(hipMemset(vc_, 0, S * L * C * E * 2));
    // RoPE table, exactly ggml's iteration (rope_tables; the context shift reads row n_discard of the same table)
    {
        std::vector<float> c, s;
        rope_tables((int)C, (int)hd, c, s);
        cos_ = takef(c.size()); sin_ = takef(s.size());
        HIP_CHECK(hipMemcpy(cos_, c.data(), c.size() * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(sin_, s.data(), s.size() * 4, hipMemcpyHostToDevice));
    }
    // fp16 lookup tables (ggml_table_gelu_f16 / silu_f16 / exp_f16), evaluated with the host libm like ggml does at init
    {
        std::vector<__half> g(65536), si(65536), ex(65536);
        for (int i = 0; i < 65536; i++) {
            const float x = __half2float(__ushort_as_half((unsigned short)i));
            g[(size_t)i] = __float2half_rn(0.5f * x * (1.0f + tanhf(0.79788456080286535587989211986876f * x * (1.0f + 0.044715f * x * x))));
            si[(size_t)i] = __float2half_rn(x / (1.0f + expf(-x)));
            ex[(size_t)i] = __float2half_rn(expf(x));
        }
        __half *dg = takeh(65536), *ds = takeh(65536), *de = takeh(65536);
        HIP_CHECK(hipMemcpy(dg, g.data(), 131072, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(ds, si.data(), 131072, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(de, ex.data(), 131072, hipMemcpyHostToDevice));
        tabs_.gelu = dg; tabs_.silu = ds; tabs_.exp = de;

        int last = 0;
        for (int i = 0; i < 0x7C00; i++) if (__half2float(ex[(size_t)(0x8000 + i)]) != 0.0f) last = i;
        tabs_.exp_neg_n = (last + 1 + 2047) / 2048 * 2048;
        tabs_dec_ = tabs_;
        if (computed_tables_) { tabs_dec_.exp = nullptr; tabs_dec_.silu = nullptr; }
        tabs_vis_ = tabs_;
        if (computed_tables_) tabs_vis_.exp = nullptr;          // the ViT / Q-Former attention of fast mode computes its exponentials (no 40 KB table DMA per workgroup)
        if (computed_tables_ && computed_gelu_) tabs_vis_.gelu = nullptr;     // ... and the GELU epilogues of its GEMMs compute the table's values (round 6)
    }
    x_ = takef(B * E); q_ = takef(B * E); k_ = takef(B * E); v_ = takef(B * E); att_ = takef(B * E);
    h1_ = takef(B * F); h3_ = takef(B * F); logits_ = takef(S * V); blogits_ = takef(S * V);
    act_.q8k = reinterpret_cast<int8_t *>(buf_arena_.take(B * Kmax)); act_.q80 = reinterpret_cast<int8_t *>(buf_arena_.take(B * Kmax));
    act_.dk = takef(B * Kmax / 256 + 16); act_.bsk = reinterpret_cast<int16_t *>(buf_arena_.take(B * Kmax / 16 * 2 + 64));
    act_.bsq = reinterpret_cast<int8_t *>(buf_arena_.take(B * Kmax / 16 + 64));
    // MINIGPT4_MMQH=1 only: fp16 images of the Q8_K rows for the fp16-MFMA prompt mat-mul (k_mmqh_q45k, not adopted)
    if (tune_.mmqh) { act_.q16 = takeh(B * Kmax); act_.bs16 = takeh(B * Kmax / 16 + 64); }
    act_.d0 = takef(B * Kmax / 32 + 16); act_.d1 = takef(B * Kmax / 32 + 16); act_.s1 = takef(B * Kmax / 32 + 16);
    act_.sum0 = reinterpret_cast<int *>(buf_arena_.take(B * Kmax / 32 * 4 + 64));
    act_.xh = takeh(B * Kmax); act_.xf = takef(B * Kmax);
    static_assert(MAX_CONVERSATIONS * 4 <= 256, "per-conversation scalars live in 256-byte slabs");
    d_npast_ = reinterpret_cast<int *>(buf_arena_.take(256)); d_argmax_ = reinterpret_cast<int *>(buf_arena_.take(256)); d_feed_ = reinterpret_cast<int *>(buf_arena_.take(256));
    d_btok_ = reinterpret_cast<int *>(buf_arena_.take(BSTAGE_BYTES)); d_bslot_ = d_btok_ + MAX_CONVERSATIONS; d_bpos_ = d_bslot_ + MAX_CONVERSATIONS;
    batch_graph_.assign((size_t)MAX_CONVERSATIONS + 1, nullptr);
    d_tokens_ = reinterpret_cast<int *>(buf_arena_.take(B * 4));
    d_scratch_ = buf_arena_.take(8192);
    attn_splits_ = attn_splits_forced_ > 0 ? attn_splits_forced_ : attn_split_count((int)llm_.n_head, tune_.cus);
    attn_ws_ = buf_arena_.take(attn_split_workspace_bytes((int)llm_.n_head, (int)hd, n_ctx_, attn_splits_));
    HIP_CHECK(hipMemset(attn_ws_, 0, attn_split_workspace_bytes((int)llm_.n_head, (int)hd, n_ctx_, attn_splits_)));   // the arrival counters start (and are left) at zero
    {   // K-split partial sums of the prefill mat-mul (only prompts short enough to need the extra parallelism use them)
        const size_t slab_floats = (size_t)16 << 20;
        act_.ws = reinterpret_cast<float *>(buf_arena_.take(slab_floats * 4)); act_.ws_floats = slab_floats;
    }
    HIP_CHECK(hipMemset(d_npast_, 0, 256)); HIP_CHECK(hipMemset(d_argmax_, 0, 256)); HIP_CHECK(hipMemset(d_feed_, 0, 256)); HIP_CHECK(hipMemset(d_btok_, 0, BSTAGE_BYTES));
    HIP_CHECK(hipMemset(d_tokens_, 0, B * 4));
    HIP_CHECK(hipHostMalloc((void **)&h_argmax_, 256, hipHostMallocDefault));
    HIP_CHECK(hipHostMalloc((void **)&h_bstage_, BSTAGE_BYTES, hipHostMallocDefault));
    HIP_CHECK(hipHostMalloc((void **)&h_logits_, V * 4, hipHostMallocDefault));
    memset(h_argmax_, 0, 256);
    // vision
    vi_img_ = takef(VB * 3 * 224 * 224); vi_patches_ = takeh(VB * 256 * 592); vi_pe_ = takef(VB * 256 * D); vi_x_ = takef(VB * 257 * D); vi_qkv_ = takef(VB * 257 * 3 * D);
    vi_slab_ = takef(VB * (size_t)SPLITK_MAX * 257 * D);
    vi_ln_h_ = takeh(VB * 257 * D); vi_att_h_ = takeh(VB * 257 * D); vi_img_h_ = takeh(VB * 257 * D); vi_mlp_h_ = takeh(VB * 257 * M);
    vi_hs_ = takef(VB * NQ * 768); vi_a1_ = takef(VB * NQ * 768); vi_a2_ = takef(VB * NQ * 768); vi_d_ = takef(VB * NQ * 768); vi_qq_ = takef(VB * NQ * 2304); vi_kv_ = takef(VB * 257 * 1536 * (size_t)std::max(1, v_ncross_));
    vi_hs_h_ = takeh(VB * NQ * 768); vi_a1_h_ = takeh(VB * NQ * 768); vi_a2_h_ = takeh(VB * NQ * 768); vi_ctx_h_ = takeh(VB * NQ * 768); vi_im_h_ = takeh(VB * NQ * (size_t)v_qi_);
    vi_out_ = takef(VB * NQ * (size_t)v_out_);
    vi_qtok_rep_ = takef(VB * NQ * 768);                                  // the query tokens once per image of a batch (every image starts from the same rows)
    // LOAD_RECV: weights_received()
    if (load_mode_ == LOAD_FULL) for (size_t b = 0; b < VB; b++) HIP_CHECK(hipMemcpy(vi_qtok_rep_ + b * NQ * 768, v_qtok_, NQ * 768 * 4, hipMemcpyDeviceToDevice));
    vi_c_a1_ = takef(VB * NQ * 768); vi_c_qq_ = takef(VB * NQ * 768); vi_c_a1_h_ = takeh(VB * NQ * 768);
    // prefill_batch: the packed chunk's tables (segments, finish rows, last rows, row table, two attention work lists) and their pinned staging
    d_seg_ = reinterpret_cast<int *>(buf_arena_.take(seg_ints() * 4));
    HIP_CHECK(hipHostMalloc((void **)&h_seg_, seg_ints() * 4, hipHostMallocDefault));
    if (v_generic_) alloc_vision_generic();
    MG4_INFO("KV cache %.1f MB (fp16, n_ctx %d, %zu conversation%s), activation arena %.1f MB", 2.0 * S * L * C * E * 2 / 1048576.0, n_ctx_, S, S == 1 ? "" : "s", buf_arena_.used / 1048576.0);
}

// ====================================================================================================================
// language path
// ====================================================================================================================
// One launch for 1..3 same-shape matrices when decoding (v2 persistent-wave kernel); otherwise one k_mul_mat launch per matrix.
// prep != null: the activation row still has to be prepared (rms_norm*w | identity | silu(a)*b + quantisation); when decoding it is fused into
// the mat-vec prologue, otherwise the standalone preparation kernel runs first.
void Engine::site_begin(const char *site, double bytes, hipStream_t s) {
    if (!prof_on_) return;
    SiteEv ev{}; ev.site = site; ev.bytes = bytes;
    HIP_CHECK(hipEventCreate(&ev.a)); HIP_CHECK(hipEventCreate(&ev.b));
    reset_kernel_name();
    ev.p0 = ev.p1 = launch_probe_count();
    HIP_CHECK(hipEventRecord(ev.a, s));
    site_events_.push_back(ev);
}
void Engine::site_end(hipStream_t s) noexcept {   // called from SiteScope's destructor: must not throw (a failed record marks the site invalid instead)
    if (!prof_on_ || site_events_.empty()) return;
    SiteEv &ev = site_events_.back();
    if (hipEventRecord(ev.b, s) != hipSuccess) { (void)hipGetLastError(); ev.bytes = -1.0; }
    ev.kernel = last_kernel_name();
    ev.p1 = launch_probe_count();
}
// rms norm * w + quantisation of N rows of x; when x is the pending result of a deferred K-split combine (x = residual + slabs), x is formed by the
// same launch
void Engine::prep_rms(const float *x, const float *w, int N, int K, int mask, hipStream_t s) {
    if (pend_.ks > 1 && pend_.n == 1 && pend_.y[0] == x && pend_.stride == (long long)N * K) { launch_rms_quant_slabs(pend_, w, N, K, act_, mask, s); pend_ = SlabSrc{}; return; }
    flush_pending(s);
    launch_rms_quant(x, w, N, K, act_, mask, s);
}
void Engine::flush_pending(hipStream_t s) { if (pend_.ks > 1) { launch_slab_flush(pend_, s); } pend_ = SlabSrc{}; }
namespace {
// how many matrices from W[from] on share its type and shape (one set launch serves such a run); same_shape: all n do
int same_run(const QWeight *const *W, int n, int from) {
    int run = 1;
    while (from + run < n && W[from + run]->type == W[from]->type && W[from + run]->rows == W[from]->rows && W[from + run]->cols == W[from]->cols) run++;
    return run;
}
bool same_shape(const QWeight *const *W, int n) { return same_run(W, n, 0) == n; }
// up to three matrices, their outputs and the residual they share, as the set launchers take them
struct WeightSet {
    const QWeight *W[3]; float *Y[3]; const float *R[3]; int n = 0;
    WeightSet(std::initializer_list<const QWeight *> Ws, std::initializer_list<float *> Ys, const float *res) {
        for (const QWeight *w : Ws) W[n++] = w;
        int i = 0; for (float *y : Ys) { Y[i] = y; R[i] = res; i++; }
    }
};
}  // namespace
bool Engine::mul_mat_set(const QWeight *const *W, float *const *y, const float *const *res, int n, int N, int ldy, hipStream_t s, const Prep *prep, bool fuse, bool silu_pair, const char *site, bool defer_ok, bool keep_pending, bool issue_bar) {
    struct ClearOverride { const __half *&p; ~ClearOverride() { p = nullptr; } } clear_override{xh_override_};   // valid for exactly one call
    const bool same = same_shape(W, n);
    int mask = 0;
    for (int i = 0; i < n; i++) mask |= act_mask_for(W[i]->type);
    const bool v2 = N == 1 && use_v2_ && same;
    fuse = fuse && v2 && prep && matvec_prologue_supported(W[0]->type, W[0]->cols);
    silu_pair = silu_pair && v2 && n == 2 && !res && matvec_silu_pair_supported(W[0]->type, W[0]->cols) && (!fuse || prep->kind == 1);
    // standalone preparation -- also the consumer of a deferred split-K combine (pend_): x = residual + slabs / silu(h1) * h3 straight from the slabs
    if (prep && !fuse) {
        SiteScope sc(this, "prepare", 0.0, s);
        const int K = W[0]->cols;
        if (prep->kind == 1) prep_rms(prep->x, prep->w, N, K, mask, s);
        else if (pend_.ks > 1 && prep->kind == 3 && pend_.n == 2 && pend_.y[0] == prep->x && pend_.y[1] == prep->w && !pend_.res[0] && !pend_.res[1] && pend_.stride == (long long)N * K) {
            launch_silu_mul_quant_slabs(pend_, N, K, act_, mask, tabs_, s); pend_ = SlabSrc{};
        } else {
            flush_pending(s);
            launch_silu_mul_quant(prep->x, prep->kind == 3 ? prep->w : nullptr, N, K, act_, mask, N == 1 ? tabs_dec_ : tabs_, s);
        }
    }
    // keep_pending (wv after a deferred wq|wk): the earlier launch's slabs stay where they are, this launch's go behind them, and both are handed to
    // the consumer together
    SlabSrc kept;
    ActQ act_here = act_;
    if (keep_pending && !prep && pend_.ks > 1 && !pend_.mixed && pend_.n == 2 && n == 1 && (size_t)pend_.n * pend_.ks * (size_t)pend_.stride < act_.ws_floats) {
        kept = pend_; pend_ = SlabSrc{};
        const size_t used = (size_t)kept.n * kept.ks * (size_t)kept.stride;
        act_here.ws += used; act_here.ws_floats -= used;
    }
    flush_pending(s);      // (nothing left unless the preparation above was fused into a mat-vec prologue or absent)
    double wbytes = 0;
    for (int i = 0; i < n; i++) wbytes += (double)W[i]->bytes;
    SiteScope sc(this, site, wbytes, s);
    bool done = false;
    // prefill: one launch for the set, weights streamed once per <= 128 rows
    if (N >= 5 && same && tune_.mmq >= 2) done = launch_mmq2_set(W, y, res, n, act_here, N, ldy, tune_, s, defer_ok && defer_combine_ ? &pend_ : nullptr);
    // the rows were left in fp16 by an earlier launch, act_ holds OTHER rows
    const bool staged_elsewhere = !prep && (xh_override_ != nullptr || (same && W[0]->type == GT_F16 && N >= 512));
    // unquantised weights at prompt sizes: the set in one launch of the big MFMA GEMM, split K for wo / w2
    if (!done && same && W[0]->type == GT_F16 && N >= 512 && act_.xh) {
        const __half *Wh[3]; for (int i = 0; i < n; i++) Wh[i] = reinterpret_cast<const __half *>(W[i]->qs);
        const __half *Ain = !prep && xh_override_ ? xh_override_ : act_.xh;     // rows some launch left in fp16 elsewhere (the feed-forward pair's epilogue)
        done = launch_gemm_f16_set(Ain, W[0]->cols, Wh, n, N, W[0]->rows, W[0]->cols, y, res, ldy, act_.ws, act_.ws_floats, tune_, s, defer_ok && defer_combine_ ? &pend_ : nullptr);
    }
    if (!done && staged_elsewhere && xh_override_) throw HipError{hipErrorInvalidValue, "F16 set launch refused rows that only exist in fp16 (no generic path may read act_ here)", __FILE__, __LINE__};
    if (!done && silu_pair) {   // the pair epilogue needs the two matrices equally spaced; launch_matvec_set refuses otherwise and the plain launch below runs
        done = fuse ? launch_matvec_set(W, y, res, n, act_, tune_, s, prep->kind, prep->x, prep->w, &tabs_, 1, issue_bar) : launch_matvec_set(W, y, res, n, act_, tune_, s, 0, nullptr, nullptr, &tabs_, 1);
        silu_pair = done;
    }
    if (!done) {
        if (fuse) done = launch_matvec_set(W, y, res, n, act_, tune_, s, prep->kind, prep->x, prep->w, &tabs_, 0, issue_bar);
        else if (v2) done = launch_matvec_set(W, y, res, n, act_, tune_, s);
    }
    if (!done) {
        if (fuse) throw HipError{hipErrorInvalidValue, "fused mat-vec prologue rejected a supported shape", __FILE__, __LINE__};
        for (int i = 0; i < n; i++) {
            const QWeight *Wp[1] = {W[i]}; float *Yp[1] = {y[i]}; const float *Rp[1] = {res ? res[i] : nullptr};
            if (!(N == 1 && use_v2_ && launch_matvec_set(Wp, Yp, Rp, 1, act_, tune_, s))) launch_mul_mat(*W[i], act_, N, y[i], ldy, res ? res[i] : nullptr, tune_, s);
        }
    }
    if (kept.ks > 1) {   // q | k pending from the earlier launch + this launch's v (pending or already in place): one SlabSrc for launch_rope_kv_slabs / the flush
        SlabSrc m = kept; m.mixed = true; m.n = 3;
        m.y[2] = y[0]; m.res[2] = res ? res[0] : nullptr;
        if (pend_.ks > 1) { m.mbase[2] = pend_.mbase[0]; m.mks[2] = pend_.mks[0]; } else { m.mbase[2] = y[0]; m.mks[2] = 1; }
        pend_ = m;
    }
    return silu_pair;
}
void Engine::mul_mat(const QWeight &W, int N, float *y, int ldy, const float *residual, hipStream_t s, const Prep *prep, bool fuse, const char *site, bool defer_ok, bool keep_pending, bool issue_bar) {
    const QWeight *Wp[1] = {&W}; float *Yp[1] = {y}; const float *Rp[1] = {residual};
    mul_mat_set(Wp, Yp, Rp, 1, N, ldy, s, prep, fuse, false, site, defer_ok, keep_pending, issue_bar);
}

// wq|wk and a differently typed wv (k-quant "more bits" layers) in one launch; returns false when the shapes / types are outside the mixed kernel's
// range.
bool Engine::mixed_qkv(const LayerW &L, hipStream_t s, bool fuse) {
    if (!use_v2_) return false;
    const int E = (int)llm_.n_embd;
    const QWeight *W1[2] = {&L.wq, &L.wk}, *W2[1] = {&L.wv}; float *Y1[2] = {q_, k_}, *Y2[1] = {v_};
    if (act_mask_for(L.wq.type) != ACT_Q8K || act_mask_for(L.wv.type) != ACT_Q8K) return false;
    SiteScope sc(this, "qkv", (double)(L.wq.bytes + L.wk.bytes + L.wv.bytes), s);   // only once the launch is certain: a refused shape must not record an empty site
    if (fuse && matvec_prologue_supported(L.wq.type, E)) { if (launch_matvec_mixed(W1, Y1, 2, W2, Y2, 1, act_, tune_, s, 1, x_, L.attn_norm, 0, mv_issue_bar_[MV_QKV_MIXED])) return true; }
    // standalone preparation, then the mixed launch; if that is refused the caller's per-type launches find the row already prepared
    launch_rms_quant(x_, L.attn_norm, 1, E, act_, ACT_Q8K, s);
    if (launch_matvec_mixed(W1, Y1, 2, W2, Y2, 1, act_, tune_, s)) return true;
    const bool keep = prof_on_; prof_on_ = false;                          // the enclosing site already covers these launches
    mul_mat_set(W1, Y1, nullptr, 2, 1, E, s, nullptr, false); mul_mat(L.wv, 1, v_, E, nullptr, s, nullptr, false);
    prof_on_ = keep;
    return true;
}

// MINIGPT4_PARITY=1 (or minigpt4_amd_set_parity): the same graph as forward() below with every fp32 accumulation in the CPU oracle's order --
// standalone row preparation (sum of squares in element order), k_mul_mat_ref (per-block terms added block after block), RoPE + cache append,
// k_attn_ref (sequential score / P.V chains), no fused prologues, no MFMA tiles.  Everything else (integer block dots, activation quantisation, fp16
// tables, RoPE table) is shared with the fast path and exact there, so this pass is BIT-IDENTICAL to oracle/refcpu.c: logits and greedy ids
// (tests/test_gpu_paritymode.py).  Slow by design (one wave per output).
void Engine::forward_ref(const Pass &p, hipStream_t s) {
    if (p.seg) throw HipError{hipErrorInvalidValue, "forward_ref: a packed chunk reached the parity pass (parity mode evaluates one conversation per pass)", __FILE__, __LINE__};
    const int N = p.N;
    const int E = (int)llm_.n_embd, F = (int)llm_.n_ff(), H = (int)llm_.n_head, hd = E / H, V = (int)llm_.n_vocab;
    const size_t C = (size_t)n_ctx_, sl = (size_t)cur_;
    int *const d_npast = d_npast_ + sl, *const d_argmax = d_argmax_ + sl, *const d_feed = d_feed_ + sl;
    float *const logits = logits_ + sl * (size_t)V;
    launch_get_rows(tok_type_, tok_raw_, E, p.feed ? d_feed : d_tokens_, N, x_, s);
    // MINIGPT4_PARITY_TRACE=<file>: every intermediate as a record {char name[32]; int64 n; float[n]} -- the oracle writes the same sequence
    // (orc_set_trace), and tools/trace_diff.py reports the first record that differs.  Synchronises after every launch; never inside a graph capture.
    auto tr = [&](const char *what, int il, const float *p, size_t n) {
        if (!trace_file_) return;
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone; HIP_IGNORE(hipStreamIsCapturing(s, &st));
        if (st != hipStreamCaptureStatusNone) return;
        std::vector<float> h(n);
        HIP_CHECK(hipMemcpyAsync(h.data(), p, n * 4, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
        char name[32]; memset(name, 0, sizeof name); snprintf(name, sizeof name, "%s.%d", what, il);
        const long long cnt = (long long)n;
        fwrite(name, 1, 32, trace_file_); fwrite(&cnt, 8, 1, trace_file_); fwrite(h.data(), 4, n, trace_file_); fflush(trace_file_);
    };
    tr("embd", -1, x_, (size_t)N * E);
    const int t_max = n_ctx_;                                              // sizes k_attn_ref's LDS rows; a captured decode step is replayed at later positions
    // one row (decode): same-type matrices of a set in one launch of the prefetching row kernel.  Prompt rows: the int8-MFMA kernels WITHOUT a K split
    // add every output's per-block terms block after block -- the oracle's order (bit-identical: test_gpu_paritymode).  Whatever those refuse (other
    // types, fewer than 5 prompt rows): the oracle-order row kernel, one generic launch per matrix
    auto ref_set = [&](std::initializer_list<const QWeight *> Ws, std::initializer_list<float *> Ys, const float *res) {
        const WeightSet m(Ws, Ys, res);
        for (int done = 0, run; done < m.n; done += run) {   // split into runs of equal type / shape (wq | wk + a differently typed wv), one launch each
            run = same_run(m.W, m.n, done);
            const float *const *R = res ? m.R + done : nullptr;
            const bool ok = N == 1 ? launch_mul_mat_ref_set(m.W + done, m.Y + done, R, run, act_, tune_, s)
                                   : N >= 5 && launch_mmq2_set(m.W + done, m.Y + done, R, run, act_, N, m.W[done]->rows, tune_, s, nullptr, 1);
            if (!ok) for (int i = 0; i < run; i++) launch_mul_mat_ref(*m.W[done + i], act_, N, m.Y[done + i], m.W[done + i]->rows, res, tune_, s);
        }
    };
    // One row without a trace (the decode step): the fast step's launch structure -- row preparation in the mat-vec prologues, wq | wk (| wv) and w1
    // | w3 as set launches -- on the oracle-order variants of the same kernels (MATVEC_EPI_REF); a set those kernels refuse (non-k-quant types) takes
    // the standalone preparation + row kernels below.
    const bool fused_row = N == 1 && !trace_file_;
    auto fused_set = [&](std::initializer_list<const QWeight *> Ws, std::initializer_list<float *> Ys, const float *res, int pro, const float *px, const float *pw) -> bool {
        if (!fused_row) return false;
        WeightSet m(Ws, Ys, res);
        if (pro != 0 && !matvec_prologue_supported(m.W[0]->type, m.W[0]->cols)) return false;
        if (same_shape(m.W, m.n)) return launch_matvec_set(m.W, m.Y, res ? m.R : nullptr, m.n, act_, tune_, s, pro, px, pw, &tabs_, MATVEC_EPI_REF);
        if (m.n == 3 && !res && same_shape(m.W, 2) && m.W[2]->cols == m.W[0]->cols && (pro == 0 || pro == 1))
            return launch_matvec_mixed(m.W, m.Y, 2, m.W + 2, m.Y + 2, 1, act_, tune_, s, pro, px, pw, MATVEC_EPI_REF);     // wq | wk + a differently typed wv
        return false;
    };
    for (size_t il = 0; il < layers_.size(); il++) {
        const LayerW &L = layers_[il];
        __half *kc = kc_ + (sl * layers_.size() + il) * C * E, *vc = vc_ + (sl * layers_.size() + il) * C * E;
        if (!fused_set({&L.wq, &L.wk, &L.wv}, {q_, k_, v_}, nullptr, 1, x_, L.attn_norm)) {
            launch_rms_quant(x_, L.attn_norm, N, E, act_, act_mask_for(L.wq.type) | act_mask_for(L.wk.type) | act_mask_for(L.wv.type), s, true);
            ref_set({&L.wq, &L.wk, &L.wv}, {q_, k_, v_}, nullptr);
        }
        tr("q", (int)il, q_, (size_t)N * E); tr("k", (int)il, k_, (size_t)N * E); tr("v", (int)il, v_, (size_t)N * E);
        // decode: RoPE + cache append inside the attention launch
        if (N == 1 && !trace_file_) launch_attn_ref_fused(q_, k_, v_, kc, vc, H, hd, d_npast, t_max, cos_, sin_, tabs_, att_, s);
        else { launch_rope_kv(q_, k_, v_, N, H, hd, d_npast, cos_, sin_, kc, vc, s); launch_attn_ref(q_, kc, vc, N, H, hd, d_npast, t_max, tabs_, att_, s); }
        tr("q_rope", (int)il, q_, (size_t)N * E); tr("att", (int)il, att_, (size_t)N * E);
        if (!fused_set({&L.wo}, {x_}, x_, 2, att_, nullptr)) {
            launch_silu_mul_quant(att_, nullptr, N, E, act_, act_mask_for(L.wo.type), tabs_, s);
            ref_set({&L.wo}, {x_}, x_);
        }
        tr("x_attn", (int)il, x_, (size_t)N * E);
        if (!fused_set({&L.w1, &L.w3}, {h1_, h3_}, nullptr, 1, x_, L.ffn_norm)) {
            launch_rms_quant(x_, L.ffn_norm, N, E, act_, act_mask_for(L.w1.type) | act_mask_for(L.w3.type), s, true);
            ref_set({&L.w1, &L.w3}, {h1_, h3_}, nullptr);
        }
        tr("h1", (int)il, h1_, (size_t)N * F); tr("h3", (int)il, h3_, (size_t)N * F);
        launch_silu_mul_quant(h1_, h3_, N, F, act_, act_mask_for(L.w2.type), tabs_, s);
        if (!fused_set({&L.w2}, {x_}, x_, 0, nullptr, nullptr)) ref_set({&L.w2}, {x_}, x_);
        tr("x_ffn", (int)il, x_, (size_t)N * E);
    }
    if (p.score) score_rows(*p.score, s);
    if (!(N == 1 && fused_set({&output_}, {logits}, nullptr, 1, x_, norm_))) {
        launch_rms_quant(x_ + (size_t)(N - 1) * E, norm_, 1, E, act_, act_mask_for(output_.type), s, true);
        const QWeight *Wo[1] = {&output_}; float *Yo[1] = {logits};
        if (!launch_mul_mat_ref_set(Wo, Yo, nullptr, 1, act_, tune_, s)) launch_mul_mat_ref(output_, act_, 1, logits, V, nullptr, tune_, s);
    }
    launch_argmax(logits, V, d_argmax, d_scratch_, s);
    launch_advance(d_npast, N, d_feed, d_argmax, s);
    HIP_CHECK(hipMemcpyAsync(h_argmax_ + sl, d_argmax, 4, hipMemcpyDeviceToHost, s));
}
void Engine::set_parity(bool on) {
    if (on == parity_) return;
    if (on && llm_.n_head > 0) {   // (advisor, round 4) the oracle-order attention kernel holds fewer keys in LDS than the fast one: refuse here, not at the first launch
        const int hd = (int)(llm_.n_embd / llm_.n_head), lim = attn_ref_max_ctx(hd);
        if (n_ctx_ > lim) throw HipError{hipErrorInvalidValue, "parity mode: n_ctx exceeds what the oracle-order attention kernel's LDS rows hold (attn_ref_max_ctx)", __FILE__, __LINE__};
        attn_ref_prepare();
    }
    HIP_CHECK(hipStreamSynchronize(stream_));
    for (Conversation &c : conv_) { if (c.graph) HIP_IGNORE(hipGraphExecDestroy(c.graph)); c.graph = nullptr; }   // captured with the other mode's launches
    for (hipGraphExec_t &g : batch_graph_) { if (g) HIP_IGNORE(hipGraphExecDestroy(g)); g = nullptr; }
    spec_drop_graphs();
    parity_ = on;
    prefix_empty();   // the store's rows were computed in the other mode
}

// Enqueue one forward pass for the p.N rows described by d_tokens_ (p.feed: the decode row, by d_feed_), at position *d_npast_.
void Engine::forward(const Pass &p, hipStream_t s) {
    pend_ = SlabSrc{}; xh_override_ = nullptr;          // host-side state of a pass that threw half-way must not reach this one
    if (parity_) { forward_ref(p, s); return; }
    const int N = p.N;
    const int E = (int)llm_.n_embd, F = (int)llm_.n_ff(), H = (int)llm_.n_head, hd = E / H, V = (int)llm_.n_vocab;
    const size_t C = (size_t)n_ctx_, sl = (size_t)cur_;                     // everything below addresses the selected conversation's cache / scalars
    int *const d_npast = d_npast_ + sl, *const d_argmax = d_argmax_ + sl, *const d_feed = d_feed_ + sl;
    float *const logits = logits_ + sl * (size_t)V;
    // p.seg (prefill_batch): the rows are the packed prompt rows of several conversations; only RoPE + cache append, the attention and the output rows change
    const SegChunk *const sg = p.seg;
    const size_t seq_stride = layers_.size() * C * (size_t)E;
    const bool dec = N == 1 && !sg;
    // feed: the row is the decode token kept in d_feed (greedy feedback / set by eval_chunk); otherwise the rows are described by d_tokens_ (id, or
    // -1 = an embedding row already sitting in x_) -- a chunk of exactly ONE embedding row must not pick up the stale decode token
    { SiteScope sc(this, "embed", (double)gt_nbytes(tok_type_, (size_t)E) * N, s); launch_get_rows(tok_type_, tok_raw_, E, p.feed ? d_feed : d_tokens_, N, x_, s); }
    auto fz = [&](int bit) { return dec && (fuse_mask_ >> bit & 1); };
    for (size_t il = 0; il < layers_.size(); il++) {
        const LayerW &L = layers_[il];
        const size_t sl_c = sg ? 0 : sl;                                     // packed rows: conversation 0's layer, the kernels add slot * seq_stride
        __half *kc = kc_ + (sl_c * layers_.size() + il) * C * E, *vc = vc_ + (sl_c * layers_.size() + il) * C * E;
        const Prep p_attn{1, x_, L.attn_norm}, p_att{2, att_, nullptr}, p_ffn{1, x_, L.ffn_norm}, p_silu{3, h1_, h3_};
        {
            const QWeight *W3[3] = {&L.wq, &L.wk, &L.wv}; float *Y3[3] = {q_, k_, v_};
            // a K-split combine is left to launch_rope_kv_slabs
            if (L.wv.type == L.wq.type) mul_mat_set(W3, Y3, nullptr, 3, N, E, s, &p_attn, fz(0), false, "qkv", !dec, false, mv_issue_bar_[MV_QKV]);
            else if (fz(6) && L.wk.type == L.wq.type && mixed_qkv(L, s, fz(0))) {}
            else if (act_mask_for(L.wv.type) == act_mask_for(L.wq.type) && !fz(0)) {   // one standalone preparation serves both launches
                prep_rms(x_, L.attn_norm, N, E, act_mask_for(L.wq.type), s);
                // both combines left to the rope launch
                mul_mat_set(W3, Y3, nullptr, 2, N, E, s, nullptr, false, false, "qk", !dec); mul_mat(L.wv, N, v_, E, nullptr, s, nullptr, false, "v", !dec, !dec);
            } else { mul_mat_set(W3, Y3, nullptr, 2, N, E, s, &p_attn, fz(0), false, "qk"); mul_mat(L.wv, N, v_, E, nullptr, s, &p_attn, fz(0), "v"); }
        }
        // algorithmic bytes of the attention site: the cached fp16 K and V rows of every head up to the current position
        bool att_in_xh = false;                                             // the attention kernel left fp16 rows in act_.xh
        std::optional<SiteScope> att_sc;
        if (prof_on_) att_sc.emplace(this, "attention", 4.0 * (double)E * (sg ? sg->key_rows : (double)(conv_[sl].n_committed + N)), s);
        if (dec && p.split) launch_attn_llm_split(q_, k_, v_, kc, vc, H, hd, d_npast, n_ctx_, cos_, sin_, tabs_dec_, att_, attn_ws_, attn_splits_, s);
        else if (dec) launch_attn_llm(q_, k_, v_, kc, vc, 1, H, hd, d_npast, n_ctx_, cos_, sin_, tabs_dec_, att_, true, s,
                                      attn_vs_ ? attn_vs_ : 4 * H <= tune_.cus ? 4 : 2 * H <= tune_.cus ? 2 : 1);   // a workgroup can need a whole CU's LDS: never more of them than CUs
        else {
            if (pend_.ks > 1 && pend_.n == 3 && pend_.y[0] == q_ && pend_.y[1] == k_ && pend_.y[2] == v_ && !pend_.res[0] && !pend_.res[1] && !pend_.res[2] && pend_.stride == (long long)N * E) {
                if (sg) launch_rope_kv_seg_slabs(pend_, N, H, hd, sg->rows, seq_stride, cos_, sin_, kc, vc, s);
                else launch_rope_kv_slabs(pend_, N, H, hd, d_npast, cos_, sin_, kc, vc, s);
                pend_ = SlabSrc{};
            } else {
                flush_pending(s);
                if (sg) launch_rope_kv_seg(q_, k_, v_, N, H, hd, sg->rows, seq_stride, cos_, sin_, kc, vc, s);
                else launch_rope_kv(q_, k_, v_, N, H, hd, d_npast, cos_, sin_, kc, vc, s);
            }
            // an F16 wo at prompt sizes multiplies fp16(attention output): let the attention kernel store those rows itself (act_.xh), no conversion
            // launch
            const bool want_h = (f16_pair_ & 4) && L.wo.type == GT_F16 && N >= 512 && act_.xh && E % 128 == 0;
            if (sg) attn_segments(*sg, kc, vc, want_h, &att_in_xh, s);
            else if (!(attn_prefill_ && launch_attn_prefill(q_, kc, vc, N, H, hd, d_npast, conv_[sl].n_committed + N, tabs_, att_, tune_, s, want_h ? act_.xh : nullptr, &att_in_xh)))
                launch_attn_llm(q_, k_, v_, kc, vc, N, H, hd, d_npast, n_ctx_, cos_, sin_, tabs_, att_, false, s);
        }
        att_sc.reset();
        mul_mat(L.wo, N, x_, E, x_, s, att_in_xh ? nullptr : &p_att, fz(1), "wo", !dec, false, mv_issue_bar_[MV_WO]);             // combine left to the ffn norm's preparation
        bool paired = false;   // h1_ already holds silu(w1 x) * (w3 x)
        // F16 weights at prompt sizes: w1 | w3 in one launch whose epilogue stores fp16(silu(w1 x) * (w3 x)) -- the rows w2 multiplies -- into h1_'s
        // memory (round 3)
        bool pair16 = false;
        if (!dec && (f16_pair_ & 1) && N >= 512 && L.w1.type == GT_F16 && L.w3.type == GT_F16 && L.w1.rows == L.w3.rows && L.w1.cols == L.w3.cols && act_.xh &&
            L.w2.type == GT_F16 && E % 128 == 0 && F % 64 == 0) {   // (w2's set launch must take the fp16 rows: its own shape conditions)
            prep_rms(x_, L.ffn_norm, N, E, act_mask_for(GT_F16), s);
            SiteScope sc(this, "w1w3", (double)(L.w1.bytes + L.w3.bytes), s);
            pair16 = launch_gemm_f16_silu_pair(act_.xh, E, reinterpret_cast<const __half *>(L.w1.qs), reinterpret_cast<const __half *>(L.w3.qs), N, F, E, pair_silu_computed_ ? tabs_dec_ : tabs_, nullptr,
                                               reinterpret_cast<__half *>(h1_), F, tune_, s);
        }
        if (pair16) {
            xh_override_ = reinterpret_cast<const __half *>(h1_);
            mul_mat(L.w2, N, x_, E, x_, s, nullptr, false, "w2", true);
            continue;
        }
        // combine left to silu * mul
        if (L.w1.type == L.w3.type) { const QWeight *W2[2] = {&L.w1, &L.w3}; float *Y2[2] = {h1_, h3_}; paired = mul_mat_set(W2, Y2, nullptr, 2, N, F, s, &p_ffn, fz(2), fz(5), "w1w3", !dec, false, mv_issue_bar_[MV_W1W3]); }
        else if (act_mask_for(L.w1.type) == act_mask_for(L.w3.type) && !fz(2)) {
            prep_rms(x_, L.ffn_norm, N, E, act_mask_for(L.w1.type), s);
            mul_mat(L.w1, N, h1_, F, nullptr, s, nullptr, false, "w1"); mul_mat(L.w3, N, h3_, F, nullptr, s, nullptr, false, "w3");
        } else { mul_mat(L.w1, N, h1_, F, nullptr, s, &p_ffn, fz(2), "w1"); mul_mat(L.w3, N, h3_, F, nullptr, s, &p_ffn, fz(2), "w3"); }
        const Prep p_h{2, h1_, nullptr};
        // combine left to the next layer's attention norm (or flushed in front of the output matrix)
        mul_mat(L.w2, N, x_, E, x_, s, paired ? &p_h : &p_silu, fz(3), "w2", !dec);
    }
    flush_pending(s);
    if (p.score) score_rows(*p.score, s);
    if (sg) {   // the last row of every conversation that ends in this chunk: one output pass over those rows, then each slot's logits / greedy id / position
        if (sg->n_end > 0) {
            launch_gather_rows(x_, sg->last, sg->n_end, E, att_, s);
            const Prep p_last{1, att_, norm_};
            mul_mat(output_, sg->n_end, blogits_, V, nullptr, s, &p_last, false, "output");
            SiteScope sc(this, "finish", (double)V * 4 * sg->n_end, s);
            launch_seg_finish(blogits_, V, sg->n_end, sg->fin, d_npast_, d_argmax_, d_feed_, logits_, s);
        }
        return;
    }
    // only the last token's logits are kept (llama.cpp logits_all = false)
    const Prep p_out{1, x_ + (size_t)(N - 1) * E, norm_};
    mul_mat(output_, 1, logits, V, nullptr, s, &p_out, fz(4), "output", false, false, mv_issue_bar_[MV_OUTPUT]);
    { SiteScope sc(this, "argmax", (double)V * 4, s); launch_argmax(logits, V, d_argmax, d_scratch_, s); }
    { SiteScope sc(this, "advance", 0.0, s); launch_advance(d_npast, N, d_feed, d_argmax, s); }
    HIP_CHECK(hipMemcpyAsync(h_argmax_ + sl, d_argmax, 4, hipMemcpyDeviceToHost, s));
}

// One decode step for B conversations at once: row r carries token d_btok_[r] of conversation d_bslot_[r].  The weights are streamed once for the B
// rows (k_mul_mat's 4-token tiles up to B = 4, the int8-MFMA kernels from B = 5); attention runs per row against its conversation's cache.  Same
// arithmetic per row as forward(1): per-row activation quantisation, exact integer block dots, the same attention kernel body.
// verify (Engine::verify_draft): the B rows are ONE conversation's (d_bslot_[0]) at consecutive positions -- the same embedding rows and mat-vec branches; the attention
// launch is launch_attn_llm_draft, the row logits go to spec_logits_ and the epilogue is launch_draft_finish.
// multi (Engine::verify_draft_batch): the B rows are consecutive groups, one per conversation, described by d_bslot_ / d_bpos_ alone -- the same embedding rows and mat-vec
// branches at B rows; the attention launch is launch_attn_llm_draft_batched, the row logits go to mspec_logits_ and the epilogue is launch_draft_finish_batch.
void Engine::forward_batch(int B, hipStream_t s, bool verify, bool epilogue, bool multi) {
    pend_ = SlabSrc{}; xh_override_ = nullptr;
    batch_path_ = BatchPath{}; batch_path_.rows = B;
    const int E = (int)llm_.n_embd, F = (int)llm_.n_ff(), H = (int)llm_.n_head, hd = E / H, V = (int)llm_.n_vocab;
    const size_t C = (size_t)n_ctx_, seq_stride = layers_.size() * C * (size_t)E;
    // y_m[t][r] = W_m[r] . act[t] (+ res_m[t][r]) for n matrices that share the prepared rows.  Up to batch_rows_max_ rows go through the pipelined
    // multi-row mat-vec in passes of 4 rows (weights streamed once per pass); larger batches / other types through launch_mul_mat (int8-MFMA tiles
    // from 5 rows). px != null: the launch prepares its rows itself (rms_norm(px_t) * pw, quantised) -- only called when rows_pro() said the shape /
    // type is in range Does the row-interleaved MFMA launch serve this set?  Every matrix of one k-quant type and shape with its image built, AND
    // where it was measured faster than the v_dot4 multi-row mat-vec (profiles/r05_batched_shapes.log, us per launch, dot4 / mfma at B = 2 | 3 | 4):
    // sets of >= 128 row groups -- qkv 17.2/15.2 | 19.8/15.2 | 23.2/15.6, wq|wk 12.4/12.9 | 14.7/12.9 | 17.1/13.2, w1|w3 25.7/22.2 | 29.6/22.1 |
    // 34.4/22.1, output 27.3/27.0 | 33.1/27.2 | 37.3/27.5 -- but not wo (80 groups: 12.3/10.7 at B = 4, less than the standalone quantisation of the
    // attention rows it would need) nor a lone wv; w2 only at B = 4 (below); and from 3 rows on: at B = 2 the v_dot4 launches prepare their rows in
    // their own prologue (two launches less per layer), which outweighs the 2-3.5 us the MFMA launch would save.
    auto ri_serves = [&](std::initializer_list<const QWeight *> Ws) {
        if (!ri_ready_ || B < 3 || B > 4) return false;
        const QWeight *w0 = *Ws.begin();
        if (!same_shape(Ws.begin(), (int)Ws.size())) return false;
        int groups = 0;
        for (const QWeight *w : Ws) { if (!ri_of(w)) return false; groups += w->rows / 64; }
        // w2 (13B: 80 row groups x 54 super-blocks): three or four workgroups share a row group, each a K range, last arriver adds the parts.  With
        // the first weight fetch ahead of the staging and batched staging loads the launch is 18.9 (Q5_K) / 20.8 us (Q6_K) against 22.8 / 22.4 for
        // the v_dot4 kernel at B = 4 (equal at B = 3): 1037 vs 1018 tok/s, alternating on one box (profiles/r05_batched_decode_inengine.log)
        if (ri_w2_ && B == 4 && Ws.size() == 1 && w0->cols >= 8192 && ri_ksplit(groups, w0->cols, ri_ws_, tune_) > 1) return true;
        return groups >= 128;
    };
    auto mm = [&](std::initializer_list<const QWeight *> Ws, std::initializer_list<float *> ys, const float *res0, int ld, const float *px = nullptr, const float *pw = nullptr) {
        WeightSet m(Ws, ys, res0);
        const int n = m.n;
        const QWeight *const *W = m.W; float *const *y = m.Y; const float *const *r = m.R;
        const bool same = same_shape(W, n);
        // wo at 3 / 4 rows (round 6, MINIGPT4_RI_WO): the attention rows are quantised as they are inside the MFMA launch (80 row groups: eight waves per workgroup split K, no
        // workgroup K split -- every workgroup stages the whole rows anyway)
        if (ri_wo_ && px && !pw && n == 1 && ri_ready_ && B >= 3 && B <= 4 && ri_of(W[0])) {
            const RiPlanes *rp[1] = {ri_of(W[0])};
            if (launch_matvec_ri(W, rp, y, res0 ? r : nullptr, 1, act_, B, ld, tune_, s, px, nullptr, W[0]->cols, RiWorkspace{})) { batch_path_.ri++; batch_path_.ri_plain++; return; }
        }
        if (ri_serves(Ws) && (!px || pw)) {                 // prepared rows, or rows this launch rms-norms and quantises itself (px, pw)
            const RiPlanes *rp[3]; for (int k = 0; k < n; k++) rp[k] = ri_of(W[k]);
            if (launch_matvec_ri(W, rp, y, res0 ? r : nullptr, n, act_, B, ld, tune_, s, px, pw, W[0]->cols, ri_ws_)) {
                batch_path_.ri++; if (ri_ksplit(n * (W[0]->rows / 64), W[0]->cols, ri_ws_, tune_) > 1) batch_path_.ri_ksplit++;
                return;
            }
        }
        if (same && B <= batch_rows_max_) {
            bool ok = true;
            for (int t0 = 0; t0 < B && ok; t0 += 4) {
                const int K = W[0]->cols;
                ActQ A = act_;
                A.q8k += (size_t)t0 * K; A.dk += (size_t)t0 * (K / 256); A.bsk += (size_t)t0 * (K / 16); A.bsq += (size_t)t0 * (K / 16); A.q80 += (size_t)t0 * K;
                A.d0 += (size_t)t0 * (K / 32); A.d1 += (size_t)t0 * (K / 32); A.s1 += (size_t)t0 * (K / 32); A.sum0 += (size_t)t0 * (K / 32);
                float *yo[3]; const float *ro[3];
                for (int k = 0; k < n; k++) { yo[k] = y[k] + (size_t)t0 * ld; ro[k] = r[k] ? r[k] + (size_t)t0 * ld : nullptr; }
                ok = launch_matvec_rows(W, yo, res0 ? ro : nullptr, n, A, std::min(4, B - t0), ld, tune_, s, px ? px + (size_t)t0 * K : nullptr, pw, K);
                if (!ok && t0) throw HipError{hipErrorInvalidValue, "multi-row mat-vec refused a pass it had accepted", __FILE__, __LINE__};
            }
            if (ok) { batch_path_.dot4++; return; }
        }
        // the launch that was to prepare its rows itself was refused (plane spacing, LDS): a performance choice must not fail the step -- prepare
        // them standalone
        if (px) {
            const int K = W[0]->cols; int mask = 0;
            for (int k = 0; k < n; k++) mask |= act_mask_for(W[k]->type);
            if (pw) launch_rms_quant(px, pw, B, K, act_, mask, s); else launch_silu_mul_quant(px, nullptr, B, K, act_, mask, tabs_, s);
        }
        for (int k = 0; k < n; k++) { launch_mul_mat(*W[k], act_, B, y[k], ld, r[k], tune_, s); batch_path_.mul_mat++; }
    };
    // may the rows of this set be prepared inside its launch?  (same conditions mm() takes the multi-row kernel under)
    auto rows_pro = [&](std::initializer_list<const QWeight *> Ws, bool plain = false) {
        // measured (profiles/r02j_batched_decode_ab.log): inside the launch the preparation pays at 2 rows (560 vs 540 tok/s) and loses at 4 (808 vs
        // 829: every fat workgroup repeats four rows' norm + quantisation); MINIGPT4_BATCH_FUSE=1 forces it for every B <= 4, =0 switches it off
        // plain = quantisation only (the attention output in front of wo: no norm, no double-precision sums): cheap enough to stay inside the launch
        // at 3 and 4 rows too
        // the MFMA launch norms + quantises its rows itself (not the plain quantisation in front of wo: wo is not served)
        if (ri_serves(Ws)) return !plain && ri_fuse_;
        if (batch_fuse_ == 0 || B > batch_rows_max_ || B > 4 || (batch_fuse_ < 0 && B > 2 && !plain)) return false;
        const QWeight *w0 = *Ws.begin();
        return same_shape(Ws.begin(), (int)Ws.size()) && matvec_rows_prologue_ok(w0->type, w0->cols);
    };
    auto attn = [&](__half *kc, __half *vc) {
        if (multi) launch_attn_llm_draft_batched(q_, k_, v_, kc, vc, B, H, hd, d_npast_, d_bslot_, d_bpos_, seq_stride, n_ctx_, cos_, sin_, tabs_dec_, att_, s);
        else if (verify) launch_attn_llm_draft(q_, k_, v_, kc, vc, B, H, hd, d_npast_, d_bslot_, seq_stride, n_ctx_, cos_, sin_, tabs_dec_, att_, s);
        else launch_attn_llm_batched(q_, k_, v_, kc, vc, B, H, hd, d_npast_, d_bslot_, seq_stride, n_ctx_, cos_, sin_, tabs_dec_, att_, s);
    };
    float *const row_logits = multi ? mspec_logits_ : verify ? spec_logits_ : blogits_;
    launch_get_rows(tok_type_, tok_raw_, E, d_btok_, B, x_, s);
    for (size_t il = 0; il < layers_.size(); il++) {
        const LayerW &L = layers_[il];
        __half *kc = kc_ + il * C * E, *vc = vc_ + il * C * E;            // conversation 0's layer; the kernel adds slot * seq_stride
        // a "more bits" layer (wq|wk Q4_K / Q5_K + wv Q6_K): one launch over both sets, like the single-row step's k_matvec_mix
        auto qkv_mixed = [&](bool pro) {
            if (!batch_mix_ || B > batch_rows_max_ || B > 4 || L.wk.type != L.wq.type || L.wv.type == L.wq.type) return false;
            const QWeight *W1[2] = {&L.wq, &L.wk}, *W2[1] = {&L.wv};
            float *y1[2] = {q_, k_}, *y2[1] = {v_};
            // at 3 and 4 prepared rows on the matrix cores (k_matvec_ri_mix), under ri_serves' conditions: every image built, >= 128 row groups in
            // the set
            if (!pro && ri_ready_ && B >= 3 && ri_of(&L.wq) && ri_of(&L.wk) && ri_of(&L.wv) && (L.wq.rows + L.wk.rows + L.wv.rows) / 64 >= 128) {
                const RiPlanes *r1[2] = {ri_of(&L.wq), ri_of(&L.wk)}, *r2[1] = {ri_of(&L.wv)};
                if (launch_matvec_ri_mixed(W1, r1, y1, 2, W2, r2, y2, 1, act_, B, E, tune_, s)) { batch_path_.ri_mix++; return true; }
            }
            const bool ok = launch_matvec_rows_mixed(W1, y1, 2, W2, y2, 1, act_, B, E, tune_, s, pro ? x_ : nullptr, pro ? L.attn_norm : nullptr, E);
            if (ok) batch_path_.dot4_mix++;
            return ok;
        };
        if (B > batch_rows_max_ && batch_sets_) {
            batch_path_.sets++;
            // More conversations than the multi-row mat-vec takes (5 ... 32): the prompt pass's launches -- one int8-MFMA launch per matrix SET, row
            // preparations that also combine a K-split predecessor (pend_), i.e. 11 launches per layer instead of the 19 of one launch + one combine
            // per matrix (round 3).
            const Prep p_attn{1, x_, L.attn_norm}, p_att{2, att_, nullptr}, p_ffn{1, x_, L.ffn_norm}, p_silu{3, h1_, h3_};
            const QWeight *W3[3] = {&L.wq, &L.wk, &L.wv}; float *Y3[3] = {q_, k_, v_};
            if (L.wv.type == L.wq.type && L.wk.type == L.wq.type) mul_mat_set(W3, Y3, nullptr, 3, B, E, s, &p_attn, false, false, "qkv");
            else {
                prep_rms(x_, L.attn_norm, B, E, act_mask_for(L.wq.type) | act_mask_for(L.wk.type) | act_mask_for(L.wv.type), s);
                if (L.wk.type == L.wq.type) { mul_mat_set(W3, Y3, nullptr, 2, B, E, s, nullptr, false, false, "qk"); mul_mat(L.wv, B, v_, E, nullptr, s, nullptr, false, "v"); }
                else { mul_mat(L.wq, B, q_, E, nullptr, s, nullptr, false, "q"); mul_mat(L.wk, B, k_, E, nullptr, s, nullptr, false, "k"); mul_mat(L.wv, B, v_, E, nullptr, s, nullptr, false, "v"); }
            }
            flush_pending(s);
            attn(kc, vc);
            mul_mat(L.wo, B, x_, E, x_, s, &p_att, false, "wo", true);
            if (L.w1.type == L.w3.type) { const QWeight *W2[2] = {&L.w1, &L.w3}; float *Y2[2] = {h1_, h3_}; mul_mat_set(W2, Y2, nullptr, 2, B, F, s, &p_ffn, false, false, "w1w3", true); }
            else { prep_rms(x_, L.ffn_norm, B, E, act_mask_for(L.w1.type) | act_mask_for(L.w3.type), s); mul_mat(L.w1, B, h1_, F, nullptr, s, nullptr, false, "w1"); mul_mat(L.w3, B, h3_, F, nullptr, s, nullptr, false, "w3"); }
            mul_mat(L.w2, B, x_, E, x_, s, &p_silu, false, "w2", true);
            continue;
        }
        if (L.wv.type == L.wq.type && L.wk.type == L.wq.type && rows_pro({&L.wq, &L.wk, &L.wv})) mm({&L.wq, &L.wk, &L.wv}, {q_, k_, v_}, nullptr, E, x_, L.attn_norm);
        else if (L.wk.type == L.wq.type && rows_pro({&L.wq, &L.wk}) && rows_pro({&L.wv})) {
            if (!qkv_mixed(true)) { mm({&L.wq, &L.wk}, {q_, k_}, nullptr, E, x_, L.attn_norm); mm({&L.wv}, {v_}, nullptr, E, x_, L.attn_norm); }
        } else {
            launch_rms_quant(x_, L.attn_norm, B, E, act_, act_mask_for(L.wq.type) | act_mask_for(L.wk.type) | act_mask_for(L.wv.type), s);
            if (L.wv.type == L.wq.type && L.wk.type == L.wq.type) mm({&L.wq, &L.wk, &L.wv}, {q_, k_, v_}, nullptr, E);
            else if (qkv_mixed(false)) {}
            else if (L.wk.type == L.wq.type) { mm({&L.wq, &L.wk}, {q_, k_}, nullptr, E); mm({&L.wv}, {v_}, nullptr, E); }
            else { mm({&L.wq}, {q_}, nullptr, E); mm({&L.wk}, {k_}, nullptr, E); mm({&L.wv}, {v_}, nullptr, E); }
        }
        attn(kc, vc);
        if (rows_pro({&L.wo}, true)) mm({&L.wo}, {x_}, x_, E, att_, nullptr);     // the attention output rows are quantised inside the wo launch
        else { launch_silu_mul_quant(att_, nullptr, B, E, act_, act_mask_for(L.wo.type), tabs_, s); mm({&L.wo}, {x_}, x_, E); }
        if (L.w1.type == L.w3.type && rows_pro({&L.w1, &L.w3})) mm({&L.w1, &L.w3}, {h1_, h3_}, nullptr, F, x_, L.ffn_norm);
        else {
            launch_rms_quant(x_, L.ffn_norm, B, E, act_, act_mask_for(L.w1.type) | act_mask_for(L.w3.type), s);
            if (L.w1.type == L.w3.type) mm({&L.w1, &L.w3}, {h1_, h3_}, nullptr, F);
            else { mm({&L.w1}, {h1_}, nullptr, F); mm({&L.w3}, {h3_}, nullptr, F); }
        }
        launch_silu_mul_quant(h1_, h3_, B, F, act_, act_mask_for(L.w2.type), tabs_dec_, s);
        // (Round 6 built the next layer's row preparation into this launch's last-arriving workgroup -- the round-5 verdict's item 3 i -- and measured 834-841 vs 994-1023 tok/s:
        // profiles/r06_batched_producer_tail.log, commit 749954e.)
        mm({&L.w2}, {x_}, x_, E);
    }
    // final norm inside the output matrix's MFMA launch
    if (B <= batch_rows_max_ && ri_fuse_ && ri_serves({&output_})) mm({&output_}, {row_logits}, nullptr, V, x_, norm_);
    else {
        prep_rms(x_, norm_, B, E, act_mask_for(output_.type), s);             // (also combines the last layer's w2 slabs when its combine was deferred)
        mm({&output_}, {row_logits}, nullptr, V);
    }
    if (multi) launch_draft_finish_batch(mspec_logits_, V, B, d_btok_, d_bslot_, d_npast_, d_argmax_, d_feed_, logits_, mspec_res_, s);
    else if (verify) { if (epilogue) launch_draft_finish(spec_logits_, V, B, d_btok_, d_bslot_, d_npast_, d_argmax_, d_feed_, logits_, spec_res_, s); }   // (the sampled form launches its own behind the pass)
    else launch_batch_finish(blogits_, V, B, d_bslot_, d_npast_, d_argmax_, d_feed_, logits_, s);
}

// What `enqueue` launches on stream_, captured and instantiated into `out` (null on entry).  A launcher that refuses a shape throws: the capture is ended all the same --
// a stream left in capture mode fails every later call with a capture error instead of the real one -- and `out` stays null.
template <class F> void Engine::capture_graph(hipGraphExec_t &out, F &&enqueue) {
    hipGraph_t g = nullptr;
    HIP_CHECK(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
    try { enqueue(); }
    catch (...) { HIP_IGNORE(hipStreamEndCapture(stream_, &g)); if (g) HIP_IGNORE(hipGraphDestroy(g)); out = nullptr; throw; }
    HIP_CHECK(hipStreamEndCapture(stream_, &g));
    HIP_CHECK(hipGraphInstantiate(&out, g, nullptr, nullptr, 0));
    HIP_CHECK(hipGraphDestroy(g));
}
size_t Engine::upload_embd_runs(const int *tok, int m, const float *embd, float *x_dst) {
    const size_t E = llm_.n_embd;
    size_t er = 0;
    for (int i = 0; i < m;) {   // contiguous runs of embedding rows go straight into the residual stream
        if (tok[i] >= 0) { i++; continue; }
        int j = i; while (j < m && tok[j] < 0) j++;
        HIP_CHECK(hipMemcpyAsync(x_dst + (size_t)i * E, embd + er * E, (size_t)(j - i) * E * 4, hipMemcpyHostToDevice, stream_));
        er += (size_t)(j - i); i = j;
    }
    return er;
}

// Evaluate one chunk of N rows of the selected conversation at its position n_committed.  row_tok[i] >= 0: token id; -1: the next packed embedding
// row of `embd`. LOAD_RECV: the arenas are allocated but hold nothing until the broadcast has landed and weights_received() ran -- every compute
// entry point refuses until then (a caller that skipped the hand-over, or an inherited MINIGPT4_LOAD=recv, must get an error, not text generated from
// uninitialised weights).
bool Engine::weights_missing() const {
    if (load_mode_ != LOAD_RECV) return false;
    set_last_error("the context was loaded in receive mode (MINIGPT4_LOAD=recv) and its weight arenas have not been filled: broadcast them, then call minigpt4_amd_weights_received");
    MG4_ERR("%s", last_error().c_str());
    return true;
}
int Engine::eval_chunk(const int *row_tok, int N, const float *embd, const ScoreReq *score) {
    if (N <= 0) return 0;
    if (weights_missing()) return 1;
    Conversation &cv = conv_[(size_t)cur_];
    launch_set_int(d_npast_ + cur_, cv.n_committed, stream_);
    if (N == 1 && row_tok[0] >= 0) {
        launch_set_int(d_feed_ + cur_, row_tok[0], stream_);
        const Pass p = decode_pass(cv, score);
        if (use_graph_ && !prof_on_ && !trace_file_ && !score) {   // a scored row runs eagerly: the same launches as the captured step + the scoring ones
            if (cv.graph && cv.graph_split != p.split) { HIP_IGNORE(hipGraphExecDestroy(cv.graph)); cv.graph = nullptr; }
            cv.graph_split = p.split;
            if (!cv.graph) capture_graph(cv.graph, [&] { forward(p, stream_); });
            HIP_CHECK(hipGraphLaunch(cv.graph, stream_));
        } else {
            forward(p, stream_);
        }
    } else {
        HIP_CHECK(hipMemcpyAsync(d_tokens_, row_tok, (size_t)N * 4, hipMemcpyHostToDevice, stream_));
        upload_embd_runs(row_tok, N, embd, x_);
        HIP_CHECK(hipStreamSynchronize(stream_));   // the (pageable) staging vectors may be reused right after this call
        Pass p{N}; p.score = score;
        forward(p, stream_);                        // k_get_rows skips rows whose id is negative
    }
    commit_rows(cur_, row_tok, N, /*past=*/false);                           // n_past counted the rows when they were queued (a caller that queued nothing adds them itself)
    return 0;
}
void Engine::commit_rows(int slot, const int *ids, int n, bool past) {
    Conversation &cv = conv_[(size_t)slot];
    cv.n_committed += n; if (past) cv.n_past += n;
    cv.has_logits = true;
    cv.hist.insert(cv.hist.end(), ids, ids + n);                             // invariant: hist.size() == n_committed
    if (logits_host_slot_ == slot) logits_host_slot_ = -1;
}

// Deferred prefill batching.  The reference evaluates every prompt fragment separately (system prompt, "Human: <Img>", the 32 image rows,
// "</Img> ", the question, "### Assistant:" -- six passes over the weights for one image turn, minigpt4.cpp:2671-2702).  Token rows do not
// depend on how they are batched (causal attention, per-row quantisation), so fragments are queued and evaluated in one pass when logits are
// needed (sampling) -- the weights are streamed once.  Context overflow is still reported by the call that would overflow.
int Engine::flush() {
    Conversation &cv = conv_[(size_t)cur_];
    if (cv.pend_tok.empty()) return 0;
    const int E = (int)llm_.n_embd;
    // prefix store (engine.hpp): a pass that starts at position 0 takes the rows the store covers from it, and may leave its own leading token run there afterwards
    const PrefixPlan plan = prefix_lookup(&cur_, 1);
    size_t er = 0;
    for (size_t i = (size_t)plan.m[0]; i < cv.pend_tok.size(); i += (size_t)max_chunk_) {   // rows below m are token rows: no embedding row is skipped
        const int n = (int)std::min((size_t)max_chunk_, cv.pend_tok.size() - i);
        size_t ne = 0; for (int k = 0; k < n; k++) ne += cv.pend_tok[i + k] < 0;
        const int rc = eval_chunk(cv.pend_tok.data() + i, n, cv.pend_embd.data() + er * E);
        er += ne;
        if (rc) { cv.drop_queue(); return rc; }
    }
    cv.pend_tok.clear(); cv.pend_embd.clear();
    prefix_commit(plan);
    return 0;
}

int Engine::set_prefix_cache(int max_rows) {
    if (max_rows < 0) { set_last_error("set_prefix_cache: max_rows < 0"); return 1; }
    max_rows = std::min(max_rows, n_ctx_);
    HIP_CHECK(hipStreamSynchronize(stream_));
    prefix_empty(); pfx_ = PrefixInfo{};
    if (max_rows == pfx_max_) return 0;
    prefix_free();
    if (max_rows == 0) return 0;
    const size_t bytes = layers_.size() * (size_t)max_rows * llm_.n_embd * sizeof(__half);
    DevPtr<__half> k(bytes), v(bytes);                                       // both or neither
    pfx_k_ = std::move(k); pfx_v_ = std::move(v);
    pfx_max_ = max_rows;
    return 0;
}
void Engine::prefix_free() { reset_all(pfx_k_, pfx_v_); pfx_max_ = 0; pfx_ids_.clear(); }
// Every listed conversation that starts at position 0 with rows queued and matches is served by ONE copy launch (n_rows = the longest match: rows above a shorter match
// are overwritten by the pass that follows on the stream); its pass then starts at row / position m
Engine::PrefixPlan Engine::prefix_lookup(const int *slots, int n) {
    PrefixPlan pl;
    if (pfx_max_ <= 0) return pl;
    for (int i = 0; i < n; i++) {
        const Conversation &cv = conv_[(size_t)slots[i]];
        if (cv.n_committed != 0 || cv.pend_tok.empty()) continue;
        pl.looked = true;
        const int run = token_run(cv), lim = std::min({run, (int)pfx_ids_.size(), (int)cv.pend_tok.size() - 1});
        int m = 0;
        while (m < lim && cv.pend_tok[(size_t)m] == pfx_ids_[(size_t)m]) m++;
        if (m >= PREFIX_MIN_ROWS) { pl.m[i] = m; pl.hit[pl.n_hit++] = slots[i]; pl.rows = std::max(pl.rows, m); pl.reused += m; }
        if (pl.cap_slot < 0 && run >= PREFIX_MIN_ROWS && m < std::min(run, pfx_max_)) { pl.cap_slot = slots[i]; pl.cap_ids.assign(cv.pend_tok.begin(), cv.pend_tok.begin() + std::min(run, pfx_max_)); }
    }
    if (pl.looked) pfx_.rows_last = 0;
    if (pl.n_hit) {
        prefix_copy_in(pl.hit, pl.n_hit, pl.rows);
        for (int i = 0; i < n; i++) if (pl.m[i]) { Conversation &cv = conv_[(size_t)slots[i]]; cv.n_committed = pl.m[i]; cv.hist.assign(cv.pend_tok.begin(), cv.pend_tok.begin() + pl.m[i]); }   // token rows: their ids are the queue's
    }
    return pl;
}
// counted, like the capture, only after every chunk of the call succeeded
void Engine::prefix_commit(const PrefixPlan &pl) {
    if (pl.n_hit) { pfx_.hits += pl.n_hit; pfx_.rows_reused_total += pl.reused; pfx_.rows_last = pl.reused; }
    if (pl.cap_slot >= 0) prefix_capture(pl.cap_slot, pl.cap_ids);
}
void Engine::prefix_copy_in(const int *slots, int n, int n_rows) {
    const size_t seq = layers_.size() * (size_t)n_ctx_ * llm_.n_embd;
    KvCopyDst d{};
    for (int i = 0; i < n; i++) { d.k[i] = kc_ + (size_t)slots[i] * seq; d.v[i] = vc_ + (size_t)slots[i] * seq; }
    launch_kv_copy(pfx_k_, pfx_v_, pfx_max_, d, n, n_ctx_, (int)layers_.size(), (int)llm_.n_embd, n_rows, stream_);
    pfx_.hit_launches++;
}
void Engine::prefix_capture(int slot, const std::vector<int> &ids) {
    const size_t seq = layers_.size() * (size_t)n_ctx_ * llm_.n_embd;
    KvCopyDst d{};
    d.k[0] = pfx_k_; d.v[0] = pfx_v_;
    prefix_empty();                                                        // a launch that fails leaves the store empty, not half-written
    launch_kv_copy(kc_ + (size_t)slot * seq, vc_ + (size_t)slot * seq, n_ctx_, d, 1, pfx_max_, (int)layers_.size(), (int)llm_.n_embd, (int)ids.size(), stream_);
    pfx_ids_ = ids;
    pfx_.captures++;
}
// The checks come before the flush, so a refused call evaluates nothing.  The copies run on stream_ behind the source's pass; a destination's captured decode step
// replays at the new position (eval_chunk writes d_npast_ and re-evaluates the key-split choice), the batched step takes positions from the host's n_committed.
int Engine::fork(int src, const int *dst, int n_dst, int n_rows) {
    const int S = (int)conv_.size();
    auto fail = [](const char *what) { set_last_error(std::string("fork_conversation: ") + what); return 1; };
    if (src < 0 || src >= S) return fail("source conversation out of range");
    if (!dst || n_dst < 1 || n_dst > S) return fail("need 1 <= n_dst <= the number of conversations");
    bool seen[MAX_CONVERSATIONS] = {false};
    for (int i = 0; i < n_dst; i++) {
        if (dst[i] < 0 || dst[i] >= S) return fail("destination conversation out of range");
        if (dst[i] == src) return fail("a destination equals the source");
        if (seen[dst[i]]) return fail("duplicate destination");
        seen[dst[i]] = true;
    }
    if (n_rows < -1 || n_rows > conv_[(size_t)src].n_past) return fail("need -1 <= n_rows <= n_past of the source");
    if (weights_missing()) return fail(last_error().c_str());
    const SelectScope restore(this);
    cur_ = src;
    Conversation &sv = conv_[(size_t)src];
    const bool whole = n_rows < 0;
    if ((whole || n_rows > sv.n_committed) && flush()) return fail(("the source's queued rows could not be evaluated: " + last_error()).c_str());
    const int rows = whole ? sv.n_committed : n_rows;
    const size_t seq = layers_.size() * (size_t)n_ctx_ * llm_.n_embd, V = llm_.n_vocab;
    KvCopyDst d{};
    for (int i = 0; i < n_dst; i++) { d.k[i] = kc_ + (size_t)dst[i] * seq; d.v[i] = vc_ + (size_t)dst[i] * seq; }
    launch_kv_copy(kc_ + (size_t)src * seq, vc_ + (size_t)src * seq, n_ctx_, d, n_dst, n_ctx_, (int)layers_.size(), (int)llm_.n_embd, rows, stream_);
    for (int i = 0; i < n_dst; i++) {
        Conversation &cv = conv_[(size_t)dst[i]];
        cv.n_committed = rows; cv.drop_queue();
        cv.hist.assign(sv.hist.begin(), sv.hist.begin() + rows);
        cv.has_logits = whole && sv.has_logits;
        if (logits_host_slot_ == dst[i]) logits_host_slot_ = -1;
        if (!whole) continue;
        HIP_CHECK(hipMemcpyAsync(logits_ + (size_t)dst[i] * V, logits_ + (size_t)src * V, V * 4, hipMemcpyDeviceToDevice, stream_));
        HIP_CHECK(hipMemcpyAsync(d_argmax_ + dst[i], d_argmax_ + src, 4, hipMemcpyDeviceToDevice, stream_));
        HIP_CHECK(hipMemcpyAsync(d_feed_ + dst[i], d_feed_ + src, 4, hipMemcpyDeviceToDevice, stream_));
    }
    if (whole) HIP_CHECK(hipMemcpyAsync(h_argmax_, d_argmax_, conv_.size() * 4, hipMemcpyDeviceToHost, stream_));   // greedy sample_token reads this copy
    return 0;
}

int Engine::add_tokens(const std::vector<int> &tokens, bool flush_now) {
    Conversation &cv = conv_[(size_t)cur_];
    const bool ids_ok = std::all_of(tokens.begin(), tokens.end(), [&](int t) { return t >= 0 && t < (int)llm_.n_vocab; });
    if (cv.n_past + (int)tokens.size() > n_ctx_ && !(ids_ok && make_room((int)tokens.size()) == 0)) {
        set_last_error("context overflow: n_past + n_tokens > n_ctx"); MG4_ERR("Failed to add string"); return E_FailedToAddString;
    }
    if (!ids_ok) { set_last_error("token id out of range"); MG4_ERR("Failed to add string"); return E_FailedToAddString; }
    cv.pend_tok.insert(cv.pend_tok.end(), tokens.begin(), tokens.end());
    cv.n_past += (int)tokens.size();
    if (flush_now || !defer_) { if (flush()) return E_FailedToAddString; }
    return E_None;
}
int Engine::add_string(const std::string &s) { return add_tokens(tok_.tokenize(s, true)); }
int Engine::add_embedding(const float *data, int n_rows) {
    Conversation &cv = conv_[(size_t)cur_];
    if (n_rows <= 0 || (cv.n_past + n_rows > n_ctx_ && make_room(n_rows))) {
        set_last_error("context overflow: n_past + n_rows > n_ctx"); MG4_ERR("Failed to add embedding"); return E_FailedToAddEmbedding;
    }
    cv.pend_tok.insert(cv.pend_tok.end(), (size_t)n_rows, -1);
    cv.pend_embd.insert(cv.pend_embd.end(), data, data + (size_t)n_rows * llm_.n_embd);
    cv.n_past += n_rows;
    if (!defer_) { if (flush()) return E_FailedToAddEmbedding; }
    return E_None;
}
// The arguments are checked against n_past before the flush (after it n_committed == n_past), so a refused call evaluates nothing and moves nothing.
// The kernel rewrites rows in place on stream_: a captured decode step replays at the new position (eval_chunk writes d_npast_, and re-captures when
// the key-split choice flips back below attn_split_t_), the batched step reads positions from d_npast_ too, parity mode shares the caches.
int Engine::shift_context(int n_keep, int n_discard) {
    Conversation &cv = conv_[(size_t)cur_];
    if (n_keep < 0 || n_discard < 0 || n_keep + n_discard > cv.n_past) {
        set_last_error("shift_context: need n_keep >= 0, n_discard >= 0 and n_keep + n_discard <= n_past"); return 1;
    }
    if (n_discard == 0) return 0;
    if (weights_missing() || flush()) return 1;
    const size_t L = layers_.size(), C = (size_t)n_ctx_, E = llm_.n_embd;
    launch_kv_shift(kc_ + (size_t)cur_ * L * C * E, vc_ + (size_t)cur_ * L * C * E, (int)L, n_ctx_, (int)E, (int)(E / llm_.n_head), n_keep, n_discard, cv.n_committed,
                    cos_, sin_, stream_);
    cv.n_committed -= n_discard; cv.n_past -= n_discard;
    cv.hist.erase(cv.hist.begin() + n_keep, cv.hist.begin() + n_keep + n_discard);
    return 0;
}
int Engine::make_room(int n) {
    Conversation &cv = conv_[(size_t)cur_];
    if (!shift_allows(n)) return 1;
    if (cv.n_past + n <= n_ctx_) return 0;
    if (flush()) return 1;
    const int need = cv.n_past + n - n_ctx_;
    return shift_context(shift_keep_, std::max(need, (cv.n_committed - shift_keep_) / 2));
}
const float *Engine::logits_host() {
    if (flush()) throw HipError{hipErrorUnknown, "deferred evaluation failed", __FILE__, __LINE__};
    if (logits_host_slot_ != cur_) {
        HIP_CHECK(hipMemcpyAsync(h_logits_, logits_ + (size_t)cur_ * llm_.n_vocab, (size_t)llm_.n_vocab * 4, hipMemcpyDeviceToHost, stream_));
        HIP_CHECK(hipStreamSynchronize(stream_));
        logits_host_slot_ = cur_;
    }
    return h_logits_;
}
int Engine::greedy_raw() {
    if (flush()) throw HipError{hipErrorUnknown, "deferred evaluation failed", __FILE__, __LINE__};
    HIP_CHECK(hipStreamSynchronize(stream_));
    return h_argmax_[cur_];                                                  // greedy: argmax computed on the device
}
int Engine::sample_token(const SampleParams &p) {
    if (p.temp <= 0) { int id = greedy_raw(); pen_pick(&cur_, 1, &id); con_pick(&cur_, 1, &id); return id; }
    if (flush()) throw HipError{hipErrorUnknown, "deferred evaluation failed", __FILE__, __LINE__};
    const Conversation &cv = conv_[(size_t)cur_];
    const float *raw = logits_host();
    const int V = (int)llm_.n_vocab;
    const bool constrained = con_handle_[cur_] && cv.has_logits;
    if (!constrained && !pen_mode_ && cv.bias_id.empty()) return sampler_.sample(raw, V, p);
    // the chain sees penalised logits, as in llama.cpp; h_logits_ (minigpt4_amd_get_logits) stays raw.  Bias, penalties, then the constraint
    pen_row_.assign(raw, raw + V);
    pen_host_row(cv, cv.hist, pen_row_.data());
    if (!constrained) return sampler_.sample(pen_row_.data(), V, p);
    // the ids outside the state's allowed set leave the chain's copy of the row
    const unsigned *allowed = con_fetch_row(con_handle_[cur_], con_state_[cur_]);
    bool any = false;
    for (int i = 0; i < V; i++) { if ((allowed[i >> 5] >> (i & 31)) & 1u) any = true; else pen_row_[(size_t)i] = -INFINITY; }
    con_info_.host_rows++;
    if (!any) { con_info_.stuck++; return CONSTRAINT_EOS; }                 // as k_constrain_pick: nothing allowed picks EOS
    const int id = sampler_.sample(pen_row_.data(), V, p);
    con_walk(cur_, id);
    return id;
}
void Engine::pen_host_row(const Conversation &cv, const std::vector<int> &hist, float *row) {
    if (!pen_mode_ && cv.bias_id.empty()) return;
    if (penalise_row(row, (int)llm_.n_vocab, hist.data(), hist.size(), pen_mode_ ? cv.pen : PenParams{}, n_ctx_, cv.bias_id.data(), cv.bias_val.data(), (int)cv.bias_id.size()))
        pen_info_.host_rows++;
}
const char *Engine::id_to_token(int id) const {
    if (id == 2) return "</s>";   // llama_token_eos()
    if (id < 0 || id >= (int)llm_.pieces.size()) return "";
    return llm_.pieces[(size_t)id].c_str();
}

int Engine::decode_loop(int steps, int *tokens_out, float *ms_total) {
    if (flush()) return 1;
    Conversation &cv = conv_[(size_t)cur_];
    if (steps <= 0 || cv.n_past + steps > n_ctx_) return 1;
    HIP_CHECK(hipStreamSynchronize(stream_));
    int first = h_argmax_[cur_];
    const Pass step = decode_pass(cv);               // the eager step below is the one eval_chunk captures (or runs) here
    if (eval_chunk(&first, 1, nullptr)) return 1;   // builds the graph if needed, d_feed_[slot] <- greedy token afterwards (k_advance)
    cv.n_past += 1;
    HIP_CHECK(hipStreamSynchronize(stream_));
    if (tokens_out) tokens_out[0] = first;
    hipEvent_t a, b; HIP_CHECK(hipEventCreate(&a)); HIP_CHECK(hipEventCreate(&b));
    HIP_CHECK(hipEventRecord(a, stream_));
    for (int i = 1; i < steps; i++) {   // step i consumes the greedy token of step i-1, left in d_tokens_[0] by k_advance
        if (tokens_out) HIP_CHECK(hipMemcpyAsync(&tokens_out[i], d_feed_ + cur_, 4, hipMemcpyDeviceToHost, stream_));
        if (cv.graph && use_graph_) HIP_CHECK(hipGraphLaunch(cv.graph, stream_)); else forward(step, stream_);
    }
    HIP_CHECK(hipEventRecord(b, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    if (ms_total) *ms_total = ms;
    HIP_IGNORE(hipEventDestroy(a)); HIP_IGNORE(hipEventDestroy(b));
    cv.n_past += steps - 1; cv.n_committed += steps - 1;
    cv.hist.back() = -1; cv.hist.insert(cv.hist.end(), (size_t)(steps - 1), -1);   // a measurement entry point: its rows' ids are not recorded
    if (logits_host_slot_ == cur_) logits_host_slot_ = -1;
    return 0;
}

int Engine::profile_sites(int steps, std::string &json) {
    if (flush()) return 1;
    Conversation &cv = conv_[(size_t)cur_];
    if (steps <= 0 || cv.n_past + steps > n_ctx_) return 1;
    HIP_CHECK(hipStreamSynchronize(stream_));
    struct ProfOff { Engine *e; ~ProfOff() { e->prof_on_ = false; kernel_name_tracing(false); } } prof_off{this};   // on every exit: a failed or throwing step included
    prof_on_ = true; kernel_name_tracing(true);
    // Every step starts behind a gate kernel that holds the stream for ~8 ms: the host queues the step's ~250 launches and ~500 event records (6-7 us
    // of host time each, more than most of the kernels run) while the gate spins, and the GPU then drains them back to back -- the event pairs time
    // kernels, not the host.
    hipEvent_t a, b; HIP_CHECK(hipEventCreate(&a)); HIP_CHECK(hipEventCreate(&b));
    int tok = h_argmax_[cur_];
    float tot = 0;
    for (int i = 0; i < steps; i++) {
        launch_delay(8000, stream_);
        HIP_CHECK(hipEventRecord(a, stream_));
        if (eval_chunk(&tok, 1, nullptr)) return 1;
        cv.n_past += 1; cv.hist.back() = -1;                                 // as decode_loop
        HIP_CHECK(hipEventRecord(b, stream_));
        HIP_CHECK(hipStreamSynchronize(stream_));
        float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, a, b)); tot += ms;
        tok = h_argmax_[cur_];
    }
    // us: dispatch begin..end (launch probes); mus: marker pairs
    struct Agg { std::string site, kernel; double us = 0, mus = 0, bytes = 0; long calls = 0; bool probed = true; };
    std::vector<Agg> agg;                                                    // first-seen order = launch order within the step
    for (auto &e : site_events_) {
        float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, e.a, e.b));
        size_t k = 0;
        while (k < agg.size() && !(agg[k].site == e.site && agg[k].kernel == e.kernel)) k++;
        if (k == agg.size()) { agg.push_back(Agg{}); agg[k].site = e.site; agg[k].kernel = e.kernel; }
        const float pus = e.p1 > e.p0 ? launch_probe_us(e.p0, e.p1) : -1.0f;
        if (pus < 0.0f) agg[k].probed = false;
        agg[k].us += pus; agg[k].mus += ms * 1e3; agg[k].bytes += e.bytes; agg[k].calls++;
        HIP_IGNORE(hipEventDestroy(e.a)); HIP_IGNORE(hipEventDestroy(e.b));
    }
    site_events_.clear();
    HIP_IGNORE(hipEventDestroy(a)); HIP_IGNORE(hipEventDestroy(b));
    char buf[768];
    json = "{\"steps\": " + std::to_string(steps) + ", \"eager_ms_per_step\": " + std::to_string(tot / steps) + ", \"sites\": [";
    for (size_t k = 0; k < agg.size(); k++) {
        // avg_us: the dispatches' own begin..end timestamps (what rocprofv3 reports); avg_us_markers: hipEventRecord pairs around the launch site
        // (adds packet processing)
        snprintf(buf, sizeof(buf), "%s{\"site\": \"%s\", \"kernel\": \"%s\", \"calls_per_step\": %.3f, \"avg_us\": %.3f, \"avg_us_markers\": %.3f, \"timing\": \"%s\", \"bytes_per_call\": %.1f}",
                 k ? ", " : "", agg[k].site.c_str(), agg[k].kernel.c_str(), (double)agg[k].calls / steps, (agg[k].probed ? agg[k].us : agg[k].mus) / (double)agg[k].calls,
                 agg[k].mus / (double)agg[k].calls, agg[k].probed ? "dispatch" : "markers", agg[k].bytes / (double)agg[k].calls);
        json += buf;
    }
    json += "]}";
    return 0;
}

// ====================================================================================================================
// several conversations per replica
// ====================================================================================================================
// The row-interleaved image of every k-quant matrix the batched step multiplies (ri_kernels.hip), built once, on the device, from the ordinary
// planes.
void Engine::build_ri_planes() {
    if (ri_ready_ || !use_ri_ || weights_missing()) return;
    std::vector<const QWeight *> ws;
    // only the sets the batched step serves this way (forward_batch: ri_serves, qkv_mixed): wq | wk | wv (of one type, or wq | wk + a Q6_K wv), w1 |
    // w3, the output matrix -- not the 80-group wo / w2
    for (const LayerW &L : layers_) {
        if (L.wk.type == L.wq.type && L.wv.type == L.wq.type) for (const QWeight *w : {&L.wq, &L.wk, &L.wv}) ws.push_back(w);
        // a "more bits" layer: k_matvec_ri_mix
        else if (L.wk.type == L.wq.type && L.wv.type == GT_Q6_K && batch_mix_) for (const QWeight *w : {&L.wq, &L.wk, &L.wv}) ws.push_back(w);
        if (L.w1.type == L.w3.type) for (const QWeight *w : {&L.w1, &L.w3}) ws.push_back(w);
    }
    if (ri_w2_) for (const LayerW &L : layers_) ws.push_back(&L.w2);
    if (ri_wo_) for (const LayerW &L : layers_) ws.push_back(&L.wo);
    ws.push_back(&output_);
    size_t total = 0;
    for (const QWeight *w : ws) { RiPlanes p; total += ri_plan(w->type, w->rows, w->cols, p, nullptr); }
    if (!total) return;
    ri_ws_.slab_floats = (size_t)1 << 18; ri_ws_.n_tickets = 1024;
    ri_arena_.alloc(total + ri_ws_.slab_floats * 4 + (size_t)ri_ws_.n_tickets * 4 + 8192);
    ri_ws_.slabs = reinterpret_cast<float *>(ri_arena_.take(ri_ws_.slab_floats * 4)); ri_ws_.tickets = reinterpret_cast<unsigned *>(ri_arena_.take((size_t)ri_ws_.n_tickets * 4));
    HIP_CHECK(hipMemset(ri_ws_.tickets, 0, (size_t)ri_ws_.n_tickets * 4));
    for (const QWeight *w : ws) {
        RiPlanes p; const size_t need = ri_plan(w->type, w->rows, w->cols, p, nullptr);
        if (!need) continue;
        ri_plan(w->type, w->rows, w->cols, p, ri_arena_.take(need));
        launch_ri_build(*w, p, stream_);
        ri_map_.emplace_back(w, p);
    }
    HIP_CHECK(hipStreamSynchronize(stream_));
    ri_ready_ = true;
    MG4_INFO("batched decode: row-interleaved image of %zu k-quant matrices, %.2f GB", ri_map_.size(), ri_arena_.used / 1e9);
}
int Engine::set_conversations(int n) {
    if (n < 1 || n > MAX_CONVERSATIONS) { set_last_error("conversation count out of range"); return 1; }
    HIP_CHECK(hipStreamSynchronize(stream_));
    release_buffers();
    beam_free();
    guide_free();
    smp_free(); smp_reseed();
    conv_.assign((size_t)n, Conversation{});
    std::fill(con_handle_, con_handle_ + MAX_CONVERSATIONS, 0); std::fill(con_state_, con_state_ + MAX_CONVERSATIONS, 0); con_assigned_ = 0;   // the compiled constraints stay
    cur_ = 0;
    prefix_empty();
    alloc_buffers();
    // the folded Q-Former constants live in the buffer arena alloc_buffers() has just re-taken (zeroed): evaluate them again, or every later encode
    // would run on all-zero layer-0 constants (round-5 advisor finding; tests/test_gpu_serve.py::test_encode_after_set_conversations_equals_fresh_context)
    if (load_mode_ == LOAD_FULL) fold_qformer_constants();
    if (n > 1 && load_mode_ == LOAD_FULL) build_ri_planes();                          // batched decode on the matrix cores needs the row-interleaved image (once per context)
    return 0;
}
int Engine::select_conversation(int slot) {
    if (slot < 0 || slot >= (int)conv_.size()) { set_last_error("conversation index out of range"); return 1; }
    cur_ = slot;
    return 0;
}
int Engine::check_slots(const int *slots, int n) const {
    const int S = (int)conv_.size();
    if (!slots || n < 1 || n > S) return 1;
    bool seen[MAX_CONVERSATIONS] = {false};
    for (int i = 0; i < n; i++) { if (slots[i] < 0 || slots[i] >= S || seen[slots[i]]) return 2; seen[slots[i]] = true; }
    return 0;
}
int Engine::decode_batch(const int *slots, int n, const SampleParams &p, int *ids_out, const int *forced, const TopOut *top) {
    const int bad = check_slots(slots, n);
    if (bad == 1 || !ids_out) { set_last_error("decode_batch: bad slot list"); return 1; }
    if (weights_missing()) return 1;
    if (bad) { set_last_error("decode_batch: conversations must be distinct and in range"); return 1; }
    if (forced) for (int i = 0; i < n; i++) if (forced[i] < 0 || forced[i] >= (int)llm_.n_vocab) { set_last_error("decode_batch: forced token id out of range"); return 1; }
    const SelectScope restore(this);
    // 1. pending prompt rows of each conversation (its own prefill pass), then sample
    // (greedy with penalties or a bias: the raw ids first, then ONE launch over the listed conversations replaces those the transformation can change)
    for (int i = 0; i < n; i++) { cur_ = slots[i]; ids_out[i] = p.temp <= 0 ? greedy_raw() : sample_token(p); }
    // (forced tokens -- minigpt4_amd_eval_batch -- neither consult nor advance a constraint)
    if (p.temp <= 0) { pen_pick(slots, n, ids_out, !forced); if (!forced) con_pick(slots, n, ids_out); }
    // 2. one weight pass for the conversations that still have room
    HIP_CHECK(hipStreamSynchronize(stream_));                                // h_bstage_ may still feed the previous step's copies
    // the report reads the rows the ids were drawn from: behind the sampling, ahead of the pass that overwrites them (one in-order stream); its copy back is queued here
    // and awaited once the step is launched
    if (top) topn_slots_launch(slots, n, top->top_n, ids_out);
    auto report = [&] { if (top) topn_slots_collect(n, top->top_n, top->top_ids, top->top_lp, top->logprob, top->rank); };
    int B = 0;
    for (int i = 0; i < n; i++) {
        Conversation &cv = conv_[(size_t)slots[i]];
        cur_ = slots[i];
        if (cv.n_past + 1 > n_ctx_ && make_room(1)) continue;               // context full (and no automatic shift): sampled, not advanced
        stage_row(B++, forced ? forced[i] : ids_out[i], slots[i], cv.n_committed);
    }
    if (!B) { report(); return 0; }
    if (parity_) {
        if (step_parity(B)) return 1;
        HIP_CHECK(hipStreamSynchronize(stream_));
        report();
        return 0;
    }
    step_begin(B);
    step_launch(B);
    for (int r = 0; r < B; r++) commit_rows(staged_slot(r), &staged_token(r), 1, /*past=*/true);
    HIP_CHECK(hipMemcpyAsync(h_argmax_, d_argmax_, conv_.size() * 4, hipMemcpyDeviceToHost, stream_));
    report();
    return 0;
}
// rows (token, conversation, position) travel in one copy; the device positions are normally current (k_advance / k_batch_finish keep them), but
// a reset may have moved the host's view, so k_batch_begin writes them like eval_chunk does
void Engine::step_begin(int B, bool verify, bool multi) {
    HIP_CHECK(hipMemcpyAsync(d_btok_, h_bstage_, BSTAGE_BYTES, hipMemcpyHostToDevice, stream_));
    if (multi) launch_mdraft_begin(d_npast_, d_bslot_, d_bpos_, B, stream_);
    else if (verify) launch_draft_begin(d_npast_, d_bslot_, d_bpos_, stream_); else launch_batch_begin(d_npast_, d_bslot_, d_bpos_, B, stream_);
}
// the step as one hipGraph per row count: token ids, conversations and positions live in device memory, so the same graph serves every set of B conversations
// and every entry point (verify: every R rows of any conversation; without its epilogue: the sampled verify pass, whose epilogue follows k_sample_rows)
void Engine::step_launch(int B, bool verify, bool epilogue, bool multi) {
    if (!use_graph_) { forward_batch(B, stream_, verify, epilogue, multi); return; }
    hipGraphExec_t &ge = (multi ? mspec_graph_ : !verify ? batch_graph_ : epilogue ? spec_graph_ : spec_sgraph_)[(size_t)B];
    if (!ge) capture_graph(ge, [&] { forward_batch(B, stream_, verify, epilogue, multi); });
    HIP_CHECK(hipGraphLaunch(ge, stream_));
}
// oracle-order arithmetic exists for the single-conversation pass only: one pass per staged row (same results as the batched step is tested to give)
int Engine::step_parity(int B) {
    for (int r = 0; r < B; r++) { cur_ = staged_slot(r); const int id = staged_token(r); if (eval_chunk(&id, 1, nullptr)) return 1; conv_[(size_t)cur_].n_past += 1; }
    return 0;
}

// ====================================================================================================================
// beam search (engine.hpp, beam.hpp)
// ====================================================================================================================
void Engine::beam_alloc() {
    if (beam_d_) return;
    DevPtr<int> d(BEAM_WORDS * 4); PinPtr<int> h(BEAM_WORDS * 4); DevPtr<float> save(((size_t)llm_.n_vocab + 2) * 4); OwnedEvent ev(0);   // all four or none
    beam_d_ = std::move(d); beam_h_ = std::move(h); beam_save_ = std::move(save); beam_ev_ = std::move(ev);
}
int Engine::beam_search(const int *slots, int n_beams, int max_tokens, float length_penalty, int n_best, int *tokens_out, int *lengths_out, float *scores_out, int *n_out, int *stats) {
    auto refuse = [](const std::string &what) { set_last_error("beam_search: " + what); return 1; };
    const int W = n_beams, V = (int)llm_.n_vocab;
    if (W < 2 || W > BEAM_MAX) return refuse("n_beams outside 2 .. 8");
    if (const int bad = check_slots(slots, W)) return refuse(bad == 1 ? "bad slot list" : "conversations must be distinct and in range");
    if (n_best < 1 || n_best > W) return refuse("n_best outside 1 .. n_beams");
    if (max_tokens < 1) return refuse("max_tokens must be at least 1");
    if (!std::isfinite(length_penalty)) return refuse("length_penalty must be finite");
    if (!tokens_out || !lengths_out || !scores_out || !n_out || !stats) return refuse("tokens_out, lengths_out, scores_out, n_out and stats are required");
    if (V <= 2 * W) return refuse("the vocabulary must hold more than 2 * n_beams tokens");
    if (weights_missing()) return refuse(last_error());
    const int src = slots[0], C = 2 * W, stride_out = max_tokens + 1;
    Conversation &sv = conv_[(size_t)src];
    if (sv.pend_tok.empty() && !sv.has_logits) return refuse("the source conversation has no current logits");
    if (n_ctx_ - sv.n_past < 1) return refuse("context full");
    const SelectScope restore(this);
    cur_ = src;
    if (flush()) return refuse("the source's queued rows could not be evaluated: " + last_error());
    if (!sv.has_logits) return refuse("the source conversation has no current logits");
    const int steps_max = std::min(max_tokens, n_ctx_ - sv.n_past), p = sv.n_committed;
    beam_alloc();
    HIP_CHECK(hipStreamSynchronize(stream_));                                // h_argmax_ is current; h_bstage_ and beam_h_ feed no earlier copy
    const int src_greedy = h_argmax_[src];
    // the source's logits row, greedy and feed token: the passes overwrite them
    HIP_CHECK(hipMemcpyAsync(beam_save_, logits_ + (size_t)src * V, (size_t)V * 4, hipMemcpyDeviceToDevice, stream_));
    HIP_CHECK(hipMemcpyAsync(beam_save_ + V, d_argmax_ + src, 4, hipMemcpyDeviceToDevice, stream_));
    HIP_CHECK(hipMemcpyAsync(beam_save_ + V + 1, d_feed_ + src, 4, hipMemcpyDeviceToDevice, stream_));
    if (fork(src, slots + 1, W - 1, -1)) return refuse(last_error());
    // inputs of every step: the listed rows of logits_, no targets, the initial scores (only beam 0 counts in the first step); the pass's rows: conversations and positions
    KvPermuteSlots ps{};
    for (int i = 0; i < BEAM_MAX; i++) {
        beam_h_[i] = i < W ? slots[i] : 0; beam_h_[8 + i] = -1; ps.s[i] = i < W ? slots[i] : 0;
        beam_h_.as<float>()[BEAM_S + i] = i == 0 ? 0.0f : -INFINITY;
    }
    HIP_CHECK(hipMemcpyAsync(beam_d_, beam_h_, 16 * 4, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipMemcpyAsync(beam_d_ + BEAM_S, beam_h_ + BEAM_S, 8 * 4, hipMemcpyHostToDevice, stream_));
    if (!parity_) {
        for (int i = 0; i < W; i++) stage_row(i, 0, slots[i], p);            // k_beam_select writes every step's tokens into d_btok_
        step_begin(W);
    }
    int *const d_ids = beam_d_ + BEAM_IDS, *const d_rank = beam_d_ + BEAM_RANK;
    float *const d_lp = reinterpret_cast<float *>(beam_d_ + BEAM_LP), *const d_tlp = reinterpret_cast<float *>(beam_d_ + BEAM_TLP), *const d_s = reinterpret_cast<float *>(beam_d_ + BEAM_S);
    BeamStep *const d_res = reinterpret_cast<BeamStep *>(beam_d_ + BEAM_RES);
    const BeamStep &hr = *reinterpret_cast<const BeamStep *>(beam_h_ + BEAM_RES);
    const size_t seq = layers_.size() * (size_t)n_ctx_ * llm_.n_embd;
    BeamBook book(W, p, length_penalty);
    for (int t = 0; t < steps_max && !book.full; t++) {
        const int pos = p + t;                                               // every listed conversation's position before this step's pass
        if (!launch_topn_rows(logits_, V, V, W, beam_d_, C, beam_d_ + 8, d_ids, d_lp, d_rank, d_tlp, stream_)) return refuse(last_error());
        if (!launch_beam_select(d_ids, d_lp, d_s, t == 0 ? 1u : (1u << W) - 1u, W, C, BEAM_EOS, V, d_res, parity_ ? d_rank : d_btok_, stream_)) return refuse(last_error());
        HIP_CHECK(hipMemcpyAsync(beam_h_ + BEAM_RES, d_res, sizeof(BeamStep), hipMemcpyDeviceToHost, stream_));
        HIP_CHECK(hipEventRecord(beam_ev_, stream_));
        launch_kv_permute(kc_, vc_, seq, (int)conv_.size(), ps, W, d_res->parent, (int)layers_.size(), n_ctx_, (int)llm_.n_embd, book.common, pos, stream_);
        if (!parity_) step_launch(W);
        HIP_CHECK(hipEventSynchronize(beam_ev_));                            // the result block; the pass is still running
        bool sane = hr.n_live == W && hr.n_fin >= 0 && hr.n_fin <= W;         // the block indexes the host's ancestry
        for (int i = 0; i < W && sane; i++) sane = hr.parent[i] >= 0 && hr.parent[i] < W && hr.tok[i] >= 0 && hr.tok[i] < V && (i >= hr.n_fin || (hr.fin_beam[i] >= 0 && hr.fin_beam[i] < W));
        if (!sane) throw HipError{hipErrorUnknown, "beam_search: the device reported a step outside the rule", __FILE__, __LINE__};
        if (parity_) {   // oracle-order arithmetic exists for the single-row pass only: one pass per beam, in slot-list order
            for (int i = 0; i < W; i++) {
                Conversation &cv = conv_[(size_t)slots[i]];
                cur_ = slots[i]; cv.n_committed = pos; cv.n_past = pos; cv.hist.resize((size_t)p);
                const int id = hr.tok[i];
                if (eval_chunk(&id, 1, nullptr)) return refuse(last_error());
            }
            cur_ = src;
        }
        book.step(hr);
    }
    book.finish();
    // the source as it was; the others as fork(n_rows = p) leaves them
    HIP_CHECK(hipMemcpyAsync(logits_ + (size_t)src * V, beam_save_, (size_t)V * 4, hipMemcpyDeviceToDevice, stream_));
    HIP_CHECK(hipMemcpyAsync(d_argmax_ + src, beam_save_ + V, 4, hipMemcpyDeviceToDevice, stream_));
    HIP_CHECK(hipMemcpyAsync(d_feed_ + src, beam_save_ + V + 1, 4, hipMemcpyDeviceToDevice, stream_));
    for (int i = 0; i < W; i++) {
        Conversation &cv = conv_[(size_t)slots[i]];
        cv.n_committed = p; cv.n_past = p; cv.hist.resize((size_t)p);
        if (i) cv.has_logits = false;
        launch_set_int(d_npast_ + slots[i], p, stream_);
        if (logits_host_slot_ == slots[i]) logits_host_slot_ = -1;
    }
    HIP_CHECK(hipMemcpyAsync(h_argmax_, d_argmax_, conv_.size() * 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    h_argmax_[src] = src_greedy;
    *n_out = book.write(n_best, stride_out, tokens_out, lengths_out, scores_out);
    for (int i = 0; i < 4; i++) stats[i] = book.stats[i];
    return 0;
}

// ====================================================================================================================
// guided decoding (engine.hpp; minigpt4_amd.h: the rule)
// ====================================================================================================================
void Engine::guide_alloc() {
    if (guide_d_) return;
    DevPtr<float> mix((size_t)GUIDE_MAX * llm_.n_vocab * 4); DevPtr<int> d(GUIDE_WORDS * 4); PinPtr<int> h(GUIDE_WORDS * 4); OwnedEvent ev(0);   // all four or none
    guide_mix_ = std::move(mix); guide_d_ = std::move(d); guide_h_ = std::move(h); guide_ev_ = std::move(ev);
}
int Engine::guide_prepare(const char *name, const int *pos, const int *neg, int n, float scale, int *all) {
    auto refuse = [&](const std::string &what) { set_last_error(std::string(name) + ": " + what); return 1; };
    if (!pos || !neg) return refuse("slots and neg_slots are required");
    if (n < 1 || n > GUIDE_MAX || 2 * n > (int)conv_.size()) return refuse("n pairs take 2 n conversations of the context, n >= 1");
    for (int i = 0; i < n; i++) { all[2 * i] = pos[i]; all[2 * i + 1] = neg[i]; }
    if (check_slots(all, 2 * n)) return refuse("the 2 n conversations must be distinct and in range");
    if (!std::isfinite(scale)) return refuse("scale must be finite");
    if (weights_missing()) return refuse(last_error());
    return logits_ready(refuse, all, 2 * n, [&] { return !prefill_batch(all, 2 * n); }) ? 0 : 1;   // one packed pass over all 2 n queues
}
template <typename Refuse, typename Evaluate> bool Engine::logits_ready(Refuse refuse, const int *slots, int n, Evaluate evaluate) {
    auto no_logits = [&]() -> int {
        for (int i = 0; i < n; i++) { const Conversation &cv = conv_[(size_t)slots[i]]; if (cv.pend_tok.empty() && !cv.has_logits) return slots[i]; }
        return -1;
    };
    int bad = no_logits();                                                    // nothing queued and nothing evaluated: known before anything runs
    if (bad < 0) { if (!evaluate()) { refuse("the queued rows could not be evaluated: " + last_error()); return false; } bad = no_logits(); }
    if (bad >= 0) { refuse("conversation " + std::to_string(bad) + " has no current logits"); return false; }
    return true;
}
template <typename Refuse> bool Engine::sampling_params_ok(Refuse refuse, float temp, int top_k, float top_p) const {
    if (!std::isfinite(temp) || !(temp > 0.0f)) { refuse("temp must be finite and > 0"); return false; }
    if (top_k < 1 || top_k > std::min(SAMPLE_MAX, (int)llm_.n_vocab)) { refuse("top_k outside 1 .. min(64, n_vocab)"); return false; }
    if (!(top_p > 0.0f) || !(top_p <= 1.0f)) { refuse("top_p outside (0, 1]"); return false; }
    return true;
}
int Engine::guided_logits(const int *pos, const int *neg, int n, float scale, float *mixed_out, int *pick_out) {
    int all[MAX_CONVERSATIONS];
    if (guide_prepare("guided_logits", pos, neg, n, scale, all)) return 1;
    const int V = (int)llm_.n_vocab;
    guide_alloc();
    HIP_CHECK(hipStreamSynchronize(stream_));                                // guide_h_ feeds no earlier copy
    GuidePair *tab = guide_h_.as<GuidePair>();
    for (int i = 0; i < n; i++) tab[i] = GuidePair{pos[i], neg[i], scale, -1, -1, {0, 0, 0}};
    HIP_CHECK(hipMemcpyAsync(guide_d_, guide_h_, (size_t)n * sizeof(GuidePair), hipMemcpyHostToDevice, stream_));
    if (!launch_guide_rows(logits_, V, V, n, guide_d_.as<const GuidePair>(), mixed_out ? guide_mix_ : nullptr, guide_d_ + GUIDE_PICK,
                           reinterpret_cast<float *>(guide_d_ + GUIDE_VAL), nullptr, stream_)) { set_last_error("guided_logits: " + last_error()); return 1; }
    guide_info_.launches++;
    HIP_CHECK(hipMemcpyAsync(guide_h_ + GUIDE_PICK, guide_d_ + GUIDE_PICK, (size_t)n * 4, hipMemcpyDeviceToHost, stream_));
    if (mixed_out) HIP_CHECK(hipMemcpyAsync(mixed_out, guide_mix_, (size_t)n * V * 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    if (pick_out) for (int i = 0; i < n; i++) pick_out[i] = guide_h_[GUIDE_PICK + i];
    return 0;
}
int Engine::decode_guided(const int *pos, const int *neg, int n, float scale, const SampleParams &p, int *ids_out) {
    auto refuse = [](const std::string &what) { set_last_error("end_chat_guided: " + what); return 1; };
    if (!ids_out) return refuse("ids_out is required");
    int all[MAX_CONVERSATIONS];
    if (guide_prepare("end_chat_guided", pos, neg, n, scale, all)) return 1;
    const SelectScope restore(this);
    const int V = (int)llm_.n_vocab;
    const bool greedy = p.temp <= 0;
    guide_alloc();
    HIP_CHECK(hipStreamSynchronize(stream_));                                // the histories are whole; h_bstage_, guide_h_ and pen_ feed no earlier copy
    // 1. how each pair's token is chosen (the kernel's pick stands / k_pen_pick on the mixed row / the host chain), from pos's history as a sample sees it: before any shift
    enum { KERNEL = 0, PEN = 1, CHAIN = 2 };
    int how[GUIDE_MAX], pen_map[GUIDE_MAX], m_pen = 0; size_t pen_off = 0;
    std::vector<PenEntry> tab;
    for (int i = 0; i < n; i++) {
        how[i] = greedy ? KERNEL : CHAIN;
        if (!greedy) continue;
        if (!pen_stage_row(conv_[(size_t)pos[i]], /*row of guide_mix_=*/i, m_pen, pen_off, tab)) continue;   // the identity
        pen_map[m_pen++] = i; how[i] = PEN;
    }
    // 2. room: both conversations of a pair advance, or neither.  The chain penalises with the history from before a shift, as decode_batch's sampling does.  Whether a shift
    // is allowed is arithmetic (shift_allows, the queue is empty, the weights are there), so a make_room that fails here is a failure on the device: thrown like any other,
    // not a refusal -- the header's "nothing changed" covers the refusals.  Conversations of earlier pairs that this loop has already shifted STAY shifted in that case
    bool adv[GUIDE_MAX];
    std::vector<std::vector<int>> hist_before((size_t)n);
    for (int i = 0; i < n; i++) {
        const bool full_p = conv_[(size_t)pos[i]].n_past + 1 > n_ctx_, full_n = conv_[(size_t)neg[i]].n_past + 1 > n_ctx_;
        adv[i] = (!full_p && !full_n) || shift_allows(1);
        if (!adv[i]) continue;
        if (full_p && how[i] == CHAIN) hist_before[(size_t)i] = conv_[(size_t)pos[i]].hist;
        for (int k = 0; k < 2; k++) {
            if (!(k ? full_n : full_p)) continue;
            cur_ = k ? neg[i] : pos[i];
            if (make_room(1)) throw HipError{hipErrorUnknown, "end_chat_guided: the automatic shift failed", __FILE__, __LINE__};
        }
    }
    // 3. the pass's rows: the pairs whose token the kernel hands over first, then those whose token the host writes (one contiguous tail of d_btok_)
    GuidePair *gt = guide_h_.as<GuidePair>();
    int B = 0, n_hand = 0, row_of[GUIDE_MAX];
    auto stage_pair = [&](int i) {
        row_of[i] = B;
        for (int k = 0; k < 2; k++) { const int sl = k ? neg[i] : pos[i]; stage_row(B++, 0, sl, conv_[(size_t)sl].n_committed); }
    };
    for (int i = 0; i < n; i++) { gt[i] = GuidePair{pos[i], neg[i], scale, -1, -1, {0, 0, 0}}; row_of[i] = -1; }
    if (!parity_) for (int i = 0; i < n; i++) if (adv[i] && how[i] == KERNEL) { stage_pair(i); gt[i].pos_tok = row_of[i]; gt[i].neg_tok = row_of[i] + 1; n_hand++; }
    const int host_row0 = B;
    for (int i = 0; i < n; i++) if (adv[i] && row_of[i] < 0) stage_pair(i);
    const bool host_first = parity_ || m_pen > 0 || !greedy;                 // some id has to reach the host before the pass can be launched
    const bool want_mixed = m_pen > 0 || !greedy;
    HIP_CHECK(hipMemcpyAsync(guide_d_, guide_h_, (size_t)n * sizeof(GuidePair), hipMemcpyHostToDevice, stream_));
    if (B && !parity_) step_begin(B);
    // 4. the decision: one launch for all pairs; the picks' copy back is awaited after the pass is launched wherever the host does not need them sooner
    if (!launch_guide_rows(logits_, V, V, n, guide_d_.as<const GuidePair>(), want_mixed ? guide_mix_ : nullptr, guide_d_ + GUIDE_PICK,
                           reinterpret_cast<float *>(guide_d_ + GUIDE_VAL), n_hand ? d_btok_ : nullptr, stream_)) return refuse(last_error());
    guide_info_.launches++; guide_info_.handed += n_hand; guide_info_.pen_picked += m_pen; guide_info_.sampled += greedy ? 0 : n;
    HIP_CHECK(hipMemcpyAsync(guide_h_ + GUIDE_PICK, guide_d_ + GUIDE_PICK, (size_t)n * 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipEventRecord(guide_ev_, stream_));
    // the kernel's picks from the pinned block; false: an id outside the vocabulary (the kernel writes none; a block that never arrived), entered as 0
    auto take_picks = [&]() -> bool {
        bool sane = true;
        for (int i = 0; i < n; i++) {
            if (how[i] != KERNEL) continue;
            ids_out[i] = guide_h_[GUIDE_PICK + i];
            if (!id_in_vocab(ids_out[i])) { sane = false; ids_out[i] = 0; }
        }
        return sane;
    };
    auto bad_pick = [] { return bad_id("end_chat_guided: the device reported an id outside the vocabulary"); };
    if (host_first) {
        if (m_pen) {
            if (!pen_launch(guide_mix_, m_pen, pen_off)) return refuse(last_error());
            pen_info_.launches++; pen_info_.last_entries = (int)pen_off;
        }
        if (!greedy) { guide_rows_.resize((size_t)n * V); HIP_CHECK(hipMemcpyAsync(guide_rows_.data(), guide_mix_, (size_t)n * V * 4, hipMemcpyDeviceToHost, stream_)); }
        HIP_CHECK(hipStreamSynchronize(stream_));
        if (!take_picks()) throw bad_pick();                                 // nothing has been launched for these picks yet
        pen_collect(m_pen, pen_map, ids_out);
        if (!greedy) for (int i = 0; i < n; i++) {                           // one draw per pair, in list order
            const Conversation &cv = conv_[(size_t)pos[i]];
            float *row = guide_rows_.data() + (size_t)i * V;
            pen_host_row(cv, hist_before[(size_t)i].empty() ? cv.hist : hist_before[(size_t)i], row);
            ids_out[i] = sampler_.sample(row, V, p);
        }
        for (int i = 0; i < n; i++) if (row_of[i] >= host_row0) staged_token(row_of[i]) = staged_token(row_of[i] + 1) = ids_out[i];
    }
    if (!B) { if (!host_first) { HIP_CHECK(hipEventSynchronize(guide_ev_)); if (!take_picks()) throw bad_pick(); } return 0; }
    // 5. the weight pass: the batched step's own (parity mode: one oracle-order single-row pass per conversation, decode_batch's fallback)
    if (parity_) {
        if (step_parity(B)) return 1;
        HIP_CHECK(hipStreamSynchronize(stream_));
        return 0;
    }
    // the tail the host chose (it synchronised to choose: the slab's copy has drained, h_bstage_ is free again)
    if (B > host_row0) HIP_CHECK(hipMemcpyAsync(d_btok_ + host_row0, &staged_token(host_row0), (size_t)(B - host_row0) * 4, hipMemcpyHostToDevice, stream_));
    step_launch(B);
    // the pass is still running.  It has advanced the device state whatever the block says: the host's book-keeping follows it before a bad block is reported
    bool sane = true;
    if (!host_first) { HIP_CHECK(hipEventSynchronize(guide_ev_)); sane = take_picks(); }
    for (int i = 0; i < n; i++) {
        if (!adv[i]) continue;
        for (int k = 0; k < 2; k++) commit_rows(k ? neg[i] : pos[i], &ids_out[i], 1, /*past=*/true);
    }
    HIP_CHECK(hipMemcpyAsync(h_argmax_, d_argmax_, conv_.size() * 4, hipMemcpyDeviceToHost, stream_));
    if (!sane) throw bad_pick();
    return 0;
}

// ---- penalties and logit bias (engine.hpp, penalty.hpp) ----
int Engine::pen_table(const Conversation &cv, std::vector<PenEntry> &tab) const {
    return pen_build_table(cv.hist.data(), cv.hist.size(), pen_mode_ ? cv.pen : PenParams{}, n_ctx_, (int)llm_.n_vocab, cv.bias_id.data(), cv.bias_val.data(), (int)cv.bias_id.size(), tab);
}
bool Engine::pen_build_row(const Conversation &cv, int row, size_t off, PenRow *out, std::vector<PenEntry> &tab) const {
    const int flags = pen_table(cv, tab);
    const PenParams pp = pen_mode_ ? cv.pen : PenParams{};
    *out = PenRow{row, (int)off, (int)tab.size(), flags, pp.repeat_penalty, pp.alpha_frequency, pp.alpha_presence, 0};
    return flags || !tab.empty();
}
bool Engine::pen_stage_row(const Conversation &cv, int row, int m, size_t &off, std::vector<PenEntry> &tab) {
    PenRow r;
    if (!pen_build_row(cv, row, off, &r, tab)) return false;
    pen_.alloc();
    pen_.rows()[m] = r;
    std::copy(tab.begin(), tab.end(), pen_.entries() + off);
    off += tab.size();
    return true;
}
bool Engine::pen_launch(const float *logits, int m, size_t n_ent) {
    const int V = (int)llm_.n_vocab;
    pen_.upload(n_ent, stream_);
    if (!launch_pen_pick(logits, V, V, m, pen_.d_rows(), pen_.d_entries(), pen_.out_d(), nullptr, stream_)) return false;
    pen_.fetch(m, sizeof(int), stream_);
    return true;
}
void Engine::pen_collect(int m, const int *map, int *ids) const {
    for (int r = 0; r < m; r++) ids[map[r]] = device_id(pen_.out_h()[r], "the penalised pick reported an id outside the vocabulary");
}
// The caller has evaluated every listed conversation's queue and synchronised (greedy_raw): hist is the whole history, the pinned staging is free.
void Engine::pen_pick(const int *slots, int n, int *ids, bool skip_constrained) {
    bool any = pen_mode_;
    for (int i = 0; i < n && !any; i++) any = !conv_[(size_t)slots[i]].bias_id.empty();
    if (!any) return;                                                        // mode off, no bias: today's path
    std::vector<PenEntry> tab;
    int m = 0, map[MAX_CONVERSATIONS]; size_t off = 0;
    for (int i = 0; i < n; i++) {
        const Conversation &cv = conv_[(size_t)slots[i]];
        if (!cv.has_logits || (skip_constrained && con_handle_[slots[i]])) continue;   // (a constrained conversation: k_constrain_pick applies its table)
        if (pen_stage_row(cv, slots[i], m, off, tab)) map[m++] = i;          // (the identity: the raw greedy id stands)
    }
    if (!m) return;
    if (!pen_launch(logits_, m, off)) throw HipError{hipErrorInvalidValue, "penalised pick launch refused", __FILE__, __LINE__};
    HIP_CHECK(hipStreamSynchronize(stream_));
    pen_collect(m, map, ids);
    pen_info_.launches++; pen_info_.last_entries = (int)off;
}
int Engine::set_conversation_penalties(int slot, const PenParams &p) {
    auto refuse = [](const char *what) { set_last_error(std::string("conversation_penalties: ") + what); return 1; };
    if (slot < 0 || slot >= (int)conv_.size()) return refuse("conversation index out of range");
    if (!std::isfinite(p.repeat_penalty) || p.repeat_penalty <= 0.0f) return refuse("repeat_penalty must be finite and > 0");
    if (!std::isfinite(p.alpha_presence) || !std::isfinite(p.alpha_frequency)) return refuse("alpha_presence and alpha_frequency must be finite");
    conv_[(size_t)slot].pen = p;
    return 0;
}
int Engine::set_logit_bias(const int *ids, const float *bias, int n) {
    auto refuse = [](const char *what) { set_last_error(std::string("set_logit_bias: ") + what); return 1; };
    if (n < 0 || n > PEN_BIAS_MAX) return refuse("n outside [0, 256]");
    if (n > 0 && (!ids || !bias)) return refuse("ids and bias are required");
    const int V = (int)llm_.n_vocab;
    std::vector<int> sorted(ids, ids + n);
    std::sort(sorted.begin(), sorted.end());
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= V) return refuse("token id out of range");
        if (bias[i] != bias[i] || bias[i] == INFINITY) return refuse("a bias must not be NaN or +infinity");
        if (i && sorted[(size_t)i] == sorted[(size_t)i - 1]) return refuse("duplicate token id");
    }
    Conversation &cv = conv_[(size_t)cur_];
    cv.bias_id.assign(ids, ids + n); cv.bias_val.assign(bias, bias + n);
    return 0;
}

// ---- constrained decoding (engine.hpp, constraint.hpp) ----
void Engine::con_alloc() {
    if (con_vocab_) return;
    const size_t V = llm_.n_vocab;
    std::vector<int> off(V + 1, 0);
    for (size_t i = 0; i < V; i++) off[i + 1] = off[i] + (int)(i < llm_.pieces.size() ? llm_.pieces[i].size() : 0);
    std::vector<unsigned char> blob((size_t)off[V] + 1, 0);
    for (size_t i = 0; i < V && i < llm_.pieces.size(); i++) std::copy(llm_.pieces[i].begin(), llm_.pieces[i].end(), blob.begin() + off[i]);
    // all four or none, the uploads included
    DevPtr<unsigned char> vocab(blob.size()); DevPtr<int> offs((V + 1) * 4);
    Stage<ConRow, int> stage; stage.alloc();
    PinPtr<unsigned> row_h((size_t)constraint_words((int)V) * 4);
    HIP_CHECK(hipMemcpy(vocab, blob.data(), blob.size(), hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(offs, off.data(), (V + 1) * 4, hipMemcpyHostToDevice));
    con_vocab_ = std::move(vocab); con_off_ = std::move(offs); con_stage_ = std::move(stage); con_row_h_ = std::move(row_h);
}
int Engine::constraint_compile(const unsigned char *pattern, long long n_bytes, int *handle) {
    auto refuse = [](const std::string &what) { set_last_error("constraint_compile: " + what); return 1; };
    if (!handle) return refuse("handle is required");
    if (!pattern) return refuse("pattern is required");
    if (weights_missing()) return refuse(last_error());
    int h = 0;
    while (h < CONSTRAINT_SLOTS && con_[h].used) h++;
    if (h == CONSTRAINT_SLOTS) return refuse("all 8 constraints of this context are in use");
    ConstraintDfa dfa; std::string err;
    if (!mg4::constraint_compile(pattern, n_bytes < 0 ? strlen(reinterpret_cast<const char *>(pattern)) : (size_t)n_bytes, dfa, err)) return refuse(err);
    con_alloc();
    const int V = (int)llm_.n_vocab, W = constraint_words(V);
    const size_t S = (size_t)dfa.n_states, t_bytes = S * 256 * 2, a_bytes = (dfa.accept.size() * 4 + 15) & ~(size_t)15, i_bytes = S * (size_t)W * 4;
    DevPtr<uint8_t> dev(t_bytes + a_bytes + i_bytes);
    try {
        HIP_CHECK(hipMemcpyAsync(dev, dfa.trans.data(), t_bytes, hipMemcpyHostToDevice, stream_));
        HIP_CHECK(hipMemcpyAsync(dev + t_bytes, dfa.accept.data(), dfa.accept.size() * 4, hipMemcpyHostToDevice, stream_));
        unsigned *index = reinterpret_cast<unsigned *>(dev + t_bytes + a_bytes);
        if (!launch_constrain_index(con_vocab_, con_off_, V, dev.as<const uint16_t>(), reinterpret_cast<const unsigned *>(dev + t_bytes), dfa.n_states, index, stream_))
            throw HipError{hipErrorInvalidValue, "constraint index launch refused", __FILE__, __LINE__};
        HIP_CHECK(hipStreamSynchronize(stream_));                            // the host vectors above go out of scope; the index is complete when the call returns
        con_[h].used = true; con_[h].dfa = std::move(dfa); con_[h].dev = std::move(dev); con_[h].index = index;
    } catch (...) { HIP_IGNORE(hipStreamSynchronize(stream_)); throw; }          // (dev is freed behind this: nothing queued reads it any more)
    con_info_.index_launches++;
    *handle = h + 1;
    return 0;
}
int Engine::constraint_free(int handle) {
    auto refuse = [](const char *what) { set_last_error(std::string("constraint_free: ") + what); return 1; };
    if (handle < 1 || handle > CONSTRAINT_SLOTS || !con_[handle - 1].used) return refuse("no such constraint");
    for (size_t i = 0; i < conv_.size(); i++) if (con_handle_[i] == handle) return refuse("a conversation uses this constraint");
    HIP_CHECK(hipStreamSynchronize(stream_));
    con_[handle - 1] = Constraint{};
    return 0;
}
int Engine::set_constraint(int slot, int handle) {
    auto refuse = [](const char *what) { set_last_error(std::string("set_constraint: ") + what); return 1; };
    if (slot < 0 || slot >= (int)conv_.size()) return refuse("conversation index out of range");
    if (handle < 0 || handle > CONSTRAINT_SLOTS || (handle && !con_[handle - 1].used)) return refuse("no such constraint");
    con_assigned_ += (handle != 0) - (con_handle_[slot] != 0);
    con_handle_[slot] = handle; con_state_[slot] = handle ? CONSTRAINT_START : 0;
    return 0;
}
void Engine::con_walk(int slot, int id) {
    if (id == CONSTRAINT_EOS || id < 0 || id >= (int)llm_.pieces.size()) return;
    const std::string &piece = llm_.pieces[(size_t)id];
    con_state_[slot] = constraint_walk(con_[con_handle_[slot] - 1].dfa.trans.data(), con_state_[slot], reinterpret_cast<const unsigned char *>(piece.data()), (int)piece.size());
}
int Engine::constraint_advance(int slot, const int *tokens, int n) {
    auto refuse = [](const std::string &what) { set_last_error("constraint_advance: " + what); return 1; };
    if (slot < 0 || slot >= (int)conv_.size()) return refuse("conversation index out of range");
    if (!con_handle_[slot]) return refuse("the conversation has no constraint");
    if (n < 0 || (n > 0 && !tokens)) return refuse("tokens is required");
    const uint16_t *trans = con_[con_handle_[slot] - 1].dfa.trans.data();
    int state = con_state_[slot];
    for (int i = 0; i < n; i++) {
        if (tokens[i] < 0 || tokens[i] >= (int)llm_.n_vocab) return refuse("token id out of range");
        if (tokens[i] == CONSTRAINT_EOS) continue;
        const std::string &piece = tokens[i] < (int)llm_.pieces.size() ? llm_.pieces[(size_t)tokens[i]] : std::string();
        state = constraint_walk(trans, state, reinterpret_cast<const unsigned char *>(piece.data()), (int)piece.size());
        if (state == CONSTRAINT_DEAD) return refuse("token " + std::to_string(i) + " leaves the pattern");
    }
    con_state_[slot] = state;
    return 0;
}
int Engine::constraint_info(int slot, int out[8]) const {
    if (!out || slot < 0 || slot >= (int)conv_.size()) { set_last_error(out ? "constraint_info: conversation index out of range" : "constraint_info: no output array"); return 1; }
    const int h = con_handle_[slot];
    out[0] = h; out[1] = con_state_[slot]; out[2] = h ? (int)con_[h - 1].dfa.accepting(con_state_[slot]) : 0; out[3] = h ? con_[h - 1].dfa.n_states : 0;
    out[4] = con_info_.launches; out[5] = con_info_.host_rows; out[6] = con_info_.stuck; out[7] = con_info_.index_launches;
    return 0;
}
const unsigned *Engine::con_fetch_row(int handle, int state) {
    const int W = constraint_words((int)llm_.n_vocab);
    HIP_CHECK(hipMemcpyAsync(con_row_h_, con_[handle - 1].index + (size_t)state * W, (size_t)W * 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    return con_row_h_;
}
int Engine::constraint_mask(int handle, int state, uint32_t *out, int n_words) {
    auto refuse = [](const char *what) { set_last_error(std::string("constraint_mask: ") + what); return 1; };
    if (handle < 1 || handle > CONSTRAINT_SLOTS || !con_[handle - 1].used) return refuse("no such constraint");
    if (state < 0 || state >= con_[handle - 1].dfa.n_states) return refuse("state out of range");
    const int W = constraint_words((int)llm_.n_vocab);
    if (!out || n_words < W) return refuse("the buffer must hold (n_vocab + 31) / 32 words rounded up to 4");
    memcpy(out, con_fetch_row(handle, state), (size_t)W * 4);
    return 0;
}
// The caller has evaluated every listed conversation's queue and synchronised (greedy_raw): hist is the whole history, the pinned staging is free.
void Engine::con_pick(const int *slots, int n, int *ids) {
    if (!con_assigned_) return;                                              // no conversation of this context holds a constraint: today's path
    std::vector<PenEntry> tab;
    int m = 0, map[MAX_CONVERSATIONS]; size_t off = 0;
    ConRow *rows = con_stage_.rows(); PenEntry *ent = con_stage_.entries();
    const int V = (int)llm_.n_vocab, W = constraint_words(V);
    for (int i = 0; i < n; i++) {
        const int slot = slots[i], h = con_handle_[slot];
        const Conversation &cv = conv_[(size_t)slot];
        if (!h || !cv.has_logits) continue;
        pen_build_row(cv, slot, off, &rows[m].pen, tab);                     // the identity included: the constraint applies whatever the table holds
        rows[m].allowed = con_[h - 1].index + (size_t)con_state_[slot] * W; rows[m].pad = 0ull;
        std::copy(tab.begin(), tab.end(), ent + off);
        off += tab.size(); map[m++] = i;
    }
    if (!m) return;
    con_stage_.upload(off, stream_);
    if (!launch_constrain_pick(logits_, V, V, m, con_stage_.d_rows(), con_stage_.d_entries(), con_stage_.out_d(), stream_))
        throw HipError{hipErrorInvalidValue, "constrained pick launch refused", __FILE__, __LINE__};
    con_stage_.fetch(m, sizeof(int), stream_);
    HIP_CHECK(hipStreamSynchronize(stream_));
    for (int r = 0; r < m; r++) {
        const int word = con_stage_.out_h()[r], id = device_id(word & ~CONSTRAIN_STUCK, "the constrained pick reported an id outside the vocabulary");
        if (word & CONSTRAIN_STUCK) con_info_.stuck++;
        ids[map[r]] = id;
        con_walk(slots[map[r]], id);
    }
    con_info_.launches++;
}
// ---- sampled batched steps decided on the device (engine.hpp, sampling.hpp) ----
int Engine::set_conversation_seed(int slot, uint64_t seed, uint64_t draws) {
    if (slot < 0 || slot >= (int)conv_.size()) { set_last_error("conversation_seed: conversation index out of range"); return 1; }
    smp_seed_[slot] = seed; smp_draws_[slot] = draws;
    return 0;
}
int Engine::sampling_info(int slot, uint64_t out[6]) const {
    if (!out || slot < 0 || slot >= (int)conv_.size()) { set_last_error(out ? "sampling_info: conversation index out of range" : "sampling_info: no output array"); return 1; }
    out[0] = smp_seed_[slot]; out[1] = smp_draws_[slot]; out[2] = smp_info_.launches; out[3] = smp_info_.handed; out[4] = smp_info_.stuck; out[5] = smp_info_.rows;
    return 0;
}
int Engine::set_conversation_mirostat(int slot, float mu) {
    if (slot < 0 || slot >= (int)conv_.size()) { set_last_error("conversation_mirostat: conversation index out of range"); return 1; }
    if (std::isinf(mu)) { set_last_error("conversation_mirostat: mu must be finite (NaN unsets it)"); return 1; }
    smp_mu_[slot] = mu;
    return 0;
}
int Engine::mirostat_info(int slot, float out[4]) const {
    if (!out || slot < 0 || slot >= (int)conv_.size()) { set_last_error(out ? "mirostat_info: conversation index out of range" : "mirostat_info: no output array"); return 1; }
    const bool set = !std::isnan(smp_mu_[slot]);
    out[0] = set ? 1.0f : 0.0f; out[1] = set ? smp_mu_[slot] : 0.0f; out[2] = smp_observed_[slot]; out[3] = smp_tau_[slot];
    return 0;
}
// the extended rule's own parameters, in the order the header lists them
template <typename Refuse> static bool chain_params_ok(Refuse refuse, const ChainParams &cp) {
    if (!(cp.tfs_z > 0.0f) || !(cp.tfs_z <= 1.0f)) { refuse("tfs_z outside (0, 1]"); return false; }
    if (!(cp.typical_p > 0.0f) || !(cp.typical_p <= 1.0f)) { refuse("typical_p outside (0, 1]"); return false; }
    if (!(cp.min_p >= 0.0f) || !(cp.min_p <= 1.0f)) { refuse("min_p outside [0, 1]"); return false; }
    if (cp.mirostat == 1) { refuse("mirostat v1 is not built"); return false; }
    if (cp.mirostat != 0 && cp.mirostat != 2) { refuse("mirostat must be 0 or 2"); return false; }
    if (!std::isfinite(cp.tau) || !(cp.tau > 0.0f)) { refuse("mirostat_tau must be finite and > 0"); return false; }
    if (!std::isfinite(cp.eta) || !(cp.eta >= 0.0f)) { refuse("mirostat_eta must be finite and >= 0"); return false; }
    return true;
}
int Engine::smp_prepare(const char *name, const int *slots, int n, float temp, int top_k, float top_p, const ChainParams *cp) {
    auto refuse = [&](const std::string &what) { set_last_error(std::string(name) + ": " + what); return 1; };
    const int bad = check_slots(slots, n);
    if (bad == 1) return refuse("bad slot list");
    if (bad) return refuse("conversations must be distinct and in range");
    if (!sampling_params_ok(refuse, temp, top_k, top_p)) return 1;
    if (cp && !chain_params_ok(refuse, *cp)) return 1;
    if (weights_missing()) return refuse(last_error());
    auto flush_each = [&] {                                                   // as decode_batch: one pass each
        const SelectScope restore(this);
        for (int i = 0; i < n; i++) { cur_ = slots[i]; if (flush()) return false; }
        return true;
    };
    return logits_ready(refuse, slots, n, flush_each) ? 0 : 1;
}
SampleRow Engine::smp_row(int slot, const PenRow &pen, int state, uint64_t draws, int tok_index, float temp, int top_k, float top_p) const {
    const int h = con_handle_[slot];
    const unsigned *allowed = h ? con_[h - 1].index + (size_t)state * constraint_words((int)llm_.n_vocab) : nullptr;
    return SampleRow{pen, allowed, temp, top_p, top_k, tok_index, smp_seed_[slot], draws};
}
template <bool EX> size_t Engine::smp_stage(const int *slots, int n, float temp, int top_k, float top_p, const ChainParams *cp) {
    auto &blk = smp_block<EX>();
    blk.alloc();
    std::vector<PenEntry> tab;
    size_t off = 0;
    for (int i = 0; i < n; i++) {
        const int slot = slots[i];
        PenRow pen;
        pen_build_row(conv_[(size_t)slot], slot, off, &pen, tab);            // the identity included: n = 0, no flags
        smp_plain(blk.rows()[i]) = smp_row(slot, pen, con_state_[slot], smp_draws_[slot], -1, temp, top_k, top_p);
        if constexpr (EX) { blk.rows()[i].chain = *cp; blk.rows()[i].chain.mu = smp_mu_[slot]; }
        std::copy(tab.begin(), tab.end(), blk.entries() + off);
        off += tab.size();
    }
    return off;
}
template <bool EX> bool Engine::smp_launch_on(const float *logits, int n, size_t n_ent, int *row_tok) {
    const int V = (int)llm_.n_vocab;
    auto &blk = smp_block<EX>();
    blk.upload(n_ent, stream_);
    if constexpr (EX) return launch_sample_rows_ex(logits, V, V, n, blk.d_rows(), blk.d_entries(), blk.out_d(), row_tok, stream_);
    else return launch_sample_rows(logits, V, V, n, blk.d_rows(), blk.d_entries(), blk.out_d(), row_tok, stream_);
}
template <bool EX> bool Engine::smp_launch(int n, size_t n_ent, bool hand) {
    if (!smp_launch_on<EX>(logits_, n, n_ent, hand ? d_btok_ : nullptr)) return false;
    smp_block<EX>().fetch(n, EX ? sizeof(SampleOutEx) : sizeof(SampleOut), stream_);
    smp_info_.launches++;
    return true;
}
template <bool EX> int Engine::sampled_candidates_t(const char *name, const int *slots, int n, float temp, int top_k, float top_p, const ChainParams *cp, int *ids_out,
                                                    float *probs_out, int *n_cand_out, int *kept_out, uint64_t *kept_mask_out) {
    if (smp_prepare(name, slots, n, temp, top_k, top_p, cp)) return 1;
    HIP_CHECK(hipStreamSynchronize(stream_));                                // the histories are whole; the block feeds no earlier copy
    auto &blk = smp_block<EX>();
    const size_t n_ent = smp_stage<EX>(slots, n, temp, top_k, top_p, cp);
    if (!smp_launch<EX>(n, n_ent, /*hand=*/false)) { set_last_error(std::string(name) + ": " + last_error()); return 1; }
    HIP_CHECK(hipEventSynchronize(blk.event()));
    for (int i = 0; i < n; i++) {
        const SampleOut &o = smp_plain(blk.out_h()[i]);
        if (ids_out) memcpy(ids_out + (size_t)i * SAMPLE_MAX, o.ids, sizeof(o.ids));
        if (probs_out) memcpy(probs_out + (size_t)i * SAMPLE_MAX, o.p, sizeof(o.p));
        if (n_cand_out) n_cand_out[i] = o.n_cand;
        if (kept_out) kept_out[i] = o.kept;
        if constexpr (EX) if (kept_mask_out) kept_mask_out[i] = (uint64_t)blk.out_h()[i].mask_lo | (uint64_t)blk.out_h()[i].mask_hi << 32;
    }
    return 0;
}
int Engine::sampled_candidates(const int *slots, int n, float temp, int top_k, float top_p, int *ids_out, float *probs_out, int *n_cand_out, int *kept_out) {
    return sampled_candidates_t<false>("sampled_candidates", slots, n, temp, top_k, top_p, nullptr, ids_out, probs_out, n_cand_out, kept_out, nullptr);
}
int Engine::sampled_candidates_ex(const int *slots, int n, float temp, int top_k, float top_p, const ChainParams &cp, int *ids_out, float *probs_out, int *n_cand_out,
                                  uint64_t *kept_mask_out) {
    return sampled_candidates_t<true>("sampled_candidates_ex", slots, n, temp, top_k, top_p, &cp, ids_out, probs_out, n_cand_out, nullptr, kept_mask_out);
}
int Engine::decode_batch_sampled(const int *slots, int n, float temp, int top_k, float top_p, int *ids_out) {
    return decode_batch_sampled_t<false>("end_chat_batch_sampled", slots, n, temp, top_k, top_p, nullptr, ids_out);
}
int Engine::decode_batch_sampled_ex(const int *slots, int n, float temp, int top_k, float top_p, const ChainParams &cp, int *ids_out) {
    return decode_batch_sampled_t<true>("end_chat_batch_sampled_ex", slots, n, temp, top_k, top_p, &cp, ids_out);
}
template <bool EX> int Engine::decode_batch_sampled_t(const char *name, const int *slots, int n, float temp, int top_k, float top_p, const ChainParams *cp, int *ids_out) {
    auto refuse = [&](const std::string &what) { set_last_error(std::string(name) + ": " + what); return 1; };
    if (!ids_out) return refuse("ids_out is required");
    if (smp_prepare(name, slots, n, temp, top_k, top_p, cp)) return 1;
    const SelectScope restore(this);
    HIP_CHECK(hipStreamSynchronize(stream_));                                // the histories are whole; h_bstage_ and the block feed no earlier copy
    // 1. the descriptors, from each history as a sample sees it: before any shift
    auto &blk = smp_block<EX>();
    const size_t n_ent = smp_stage<EX>(slots, n, temp, top_k, top_p, cp);
    auto *rows = blk.rows();
    // 2. room, and the pass's rows: a conversation that is full and cannot shift is sampled and reported, not advanced
    int B = 0, row_of[MAX_CONVERSATIONS];
    for (int i = 0; i < n; i++) {
        Conversation &cv = conv_[(size_t)slots[i]];
        cur_ = slots[i]; row_of[i] = -1;
        if (cv.n_past + 1 > n_ctx_ && make_room(1)) continue;
        row_of[i] = B; stage_row(B++, 0, slots[i], cv.n_committed);
        if (!parity_) smp_plain(rows[i]).tok_index = row_of[i];
    }
    const bool hand = B > 0 && !parity_;
    if (hand) step_begin(B);
    // 3. the decision: one launch for all listed conversations; the picks of those that advance go straight into the pass's row tokens
    if (!smp_launch<EX>(n, n_ent, hand)) return refuse(last_error());
    smp_info_.rows += (uint64_t)n; smp_info_.handed += hand ? (uint64_t)B : 0;
    // the block from pinned memory; false: an id outside the vocabulary (the kernel writes none; a block that never arrived), entered as 0
    auto take_picks = [&]() -> bool {
        bool sane = true;
        for (int i = 0; i < n; i++) {
            ids_out[i] = smp_plain(blk.out_h()[i]).pick;
            if (!id_in_vocab(ids_out[i])) { sane = false; ids_out[i] = 0; }
        }
        return sane;
    };
    // the sampler's own state follows every decision, whether or not the conversation advances
    auto sampler_state = [&] {
        for (int i = 0; i < n; i++) {
            smp_draws_[slots[i]] += 1;
            if (smp_plain(blk.out_h()[i]).stuck == 1) smp_info_.stuck++;
            if constexpr (EX) if (cp->mirostat == 2) { smp_mu_[slots[i]] = blk.out_h()[i].mu; smp_observed_[slots[i]] = blk.out_h()[i].observed; smp_tau_[slots[i]] = cp->tau; }
            if (con_handle_[slots[i]]) con_walk(slots[i], ids_out[i]);
        }
    };
    auto bad_pick = [] {
        return bad_id(EX ? "end_chat_batch_sampled_ex: the device reported an id outside the vocabulary" : "end_chat_batch_sampled: the device reported an id outside the vocabulary");
    };
    if (!hand) {                                                             // parity mode, or nobody advances: the picks first
        HIP_CHECK(hipEventSynchronize(blk.event()));
        if (!take_picks()) throw bad_pick();                                 // nothing has been launched for these picks yet
        sampler_state();
        if (!B) return 0;
        for (int i = 0; i < n; i++) if (row_of[i] >= 0) staged_token(row_of[i]) = ids_out[i];
        if (step_parity(B)) return 1;
        HIP_CHECK(hipStreamSynchronize(stream_));
        return 0;
    }
    // 4. the weight pass: the batched step's own.  It advances the device state whatever the block says: the host's book-keeping follows it before a bad block is reported
    step_launch(B);
    HIP_CHECK(hipEventSynchronize(blk.event()));
    const bool sane = take_picks();
    sampler_state();
    for (int i = 0; i < n; i++) if (row_of[i] >= 0) commit_rows(slots[i], &ids_out[i], 1, /*past=*/true);
    HIP_CHECK(hipMemcpyAsync(h_argmax_, d_argmax_, conv_.size() * 4, hipMemcpyDeviceToHost, stream_));
    if (!sane) throw bad_pick();
    return 0;
}
int Engine::token_history(int *out, int cap) {
    if (flush()) return -1;
    const Conversation &cv = conv_[(size_t)cur_];
    if (out) for (int i = 0; i < cap && i < (int)cv.hist.size(); i++) out[i] = cv.hist[(size_t)i];
    return (int)cv.hist.size();
}

// ---- snapshots (engine.hpp, state.hpp) ----
void Engine::state_alloc(size_t block_bytes) {
    const size_t words = (size_t)n_ctx_ + 1;                                 // a block holds at least one row: at most n_ctx checksums, then the greedy | feed word
    if (state_cap_ >= block_bytes && state_sum_words_ >= words && state_cs_) return;
    HIP_CHECK(hipStreamSynchronize(stream_));                                // nothing queued may still use what is replaced
    const size_t cap = std::max(block_bytes, state_cap_), nw = std::max(words, state_sum_words_);
    DevPtr<__half> d0(cap), d1(cap); PinPtr<uint8_t> h0(cap), h1(cap);       // all or nothing: locals first
    DevPtr<unsigned long long> sd(nw * 8); PinPtr<unsigned long long> sh(nw * 8);
    if (!state_cs_) {
        OwnedStream cs(0); OwnedEvent k0(0), k1(0), c0(0), c1(0);
        state_cs_ = std::move(cs); state_ev_kernel_[0] = std::move(k0); state_ev_kernel_[1] = std::move(k1); state_ev_copy_[0] = std::move(c0); state_ev_copy_[1] = std::move(c1);
    }
    state_d_[0] = std::move(d0); state_d_[1] = std::move(d1); state_h_[0] = std::move(h0); state_h_[1] = std::move(h1); state_sum_d_ = std::move(sd); state_sum_h_ = std::move(sh);
    state_cap_ = cap; state_sum_words_ = nw;
    state_info_.staging_bytes = (long long)(4 * cap + 16 * nw);
}
int Engine::state_header(int slot, StateHeader &h, StateLayout &l) const {
    const Conversation &cv = conv_[(size_t)slot];
    h = StateHeader{};
    h.n_layer = (uint32_t)layers_.size(); h.n_embd = (uint32_t)llm_.n_embd; h.n_head = (uint32_t)llm_.n_head; h.n_vocab = (uint32_t)llm_.n_vocab;
    h.arena_hash = llm_arena_.layout_hash;
    h.n_rows = (uint32_t)cv.n_past;
    h.block_rows = state_block_rows(state_block_bytes_, state_row_bytes(h.n_layer, h.n_embd));
    h.flags = ((cv.has_logits || !cv.pend_tok.empty()) ? STATE_HAS_LOGITS : 0u) | (parity_ ? STATE_PARITY : 0u);   // queued rows: their pass leaves logits
    h.n_bias = (uint32_t)cv.bias_id.size();
    std::string why;
    if (!state_layout(h, l, why)) { set_last_error("state_save: " + why); return 1; }
    h.total_bytes = l.total;
    return 0;
}
size_t Engine::state_size(int slot) {
    if (slot < 0 || slot >= (int)conv_.size()) { set_last_error("state_size: conversation index out of range"); return 0; }
    StateHeader h; StateLayout l;
    return state_header(slot, h, l) ? 0 : l.total;
}
int Engine::state_save(int slot, void *buf, size_t cap, size_t *written) {
    auto fail = [](const std::string &what) { set_last_error("state_save: " + what); return 1; };
    if (written) *written = 0;
    if (slot < 0 || slot >= (int)conv_.size()) return fail("conversation index out of range");
    StateHeader h; StateLayout l;
    if (state_header(slot, h, l)) return 1;
    if (written) *written = l.total;
    if (!buf || cap < l.total) return fail("the buffer holds " + std::to_string(buf ? cap : 0) + " bytes, the snapshot takes " + std::to_string(l.total));
    if (weights_missing()) return fail(last_error());
    const SelectScope restore(this);
    cur_ = slot;
    if (flush()) { if (written) *written = 0; return fail("the queued rows could not be evaluated: " + last_error()); }
    const Conversation &cv = conv_[(size_t)slot];                            // n_committed == n_past == h.n_rows, has_logits as the header says
    const int L = (int)h.n_layer, E = (int)h.n_embd, V = (int)h.n_vocab;
    const size_t seq = (size_t)L * n_ctx_ * E;
    state_alloc((size_t)std::min(h.block_rows, std::max(h.n_rows, 1u)) * l.row_bytes);
    uint8_t *out = static_cast<uint8_t *>(buf);
    for (uint32_t r = 0; r < h.n_rows; r++) state_put32(out + l.hist + (size_t)4 * r, (uint32_t)cv.hist[r]);
    if (h.flags & STATE_HAS_LOGITS) memcpy(out + l.logits, logits_host(), (size_t)V * 4);   // (little-endian hosts only, like the model files)
    uint8_t *pp = out + l.pen;
    state_put32(pp, (uint32_t)cv.pen.repeat_last_n); memcpy(pp + 4, &cv.pen.repeat_penalty, 4); memcpy(pp + 8, &cv.pen.alpha_presence, 4); memcpy(pp + 12, &cv.pen.alpha_frequency, 4);
    state_put32(pp + 16, (uint32_t)cv.pen.penalize_nl);
    for (uint32_t b = 0; b < h.n_bias; b++) { state_put32(out + l.bias + (size_t)8 * b, (uint32_t)cv.bias_id[b]); memcpy(out + l.bias + (size_t)8 * b + 4, &cv.bias_val[b], 4); }
    memset(out + l.bias + (size_t)8 * h.n_bias, 0, l.table - (l.bias + (size_t)8 * h.n_bias));
    memset(out + l.table + (size_t)8 * l.n_blocks, 0, l.kv - (l.table + (size_t)8 * l.n_blocks));
    // the blocks: pack c + 1 on stream_ while block c's copy (copy stream) and the memcpy below run.  Staging block i is reused by block c + 2: its pack is issued after the
    // host has waited for block c's copy, so neither the device block nor the pinned one is overwritten early
    auto issue = [&](uint32_t c) {
        const int i = (int)(c & 1), r0 = (int)(c * h.block_rows), n = (int)state_rows_of_block(h, c);
        launch_kv_pack(kc_ + (size_t)slot * seq, vc_ + (size_t)slot * seq, n_ctx_, L, E, r0, n, state_d_[i], state_sum_d_ + c, stream_);
        state_info_.pack_launches++;
        HIP_CHECK(hipEventRecord(state_ev_kernel_[i], stream_));
        HIP_CHECK(hipStreamWaitEvent(state_cs_, state_ev_kernel_[i], 0));
        HIP_CHECK(hipMemcpyAsync(state_h_[i], state_d_[i], (size_t)n * l.row_bytes, hipMemcpyDeviceToHost, state_cs_));
        HIP_CHECK(hipEventRecord(state_ev_copy_[i], state_cs_));
    };
    if (l.n_blocks) issue(0);
    size_t off = l.kv;
    for (uint32_t c = 0; c < l.n_blocks; c++) {
        if (c + 1 < l.n_blocks) issue(c + 1);
        HIP_CHECK(hipEventSynchronize(state_ev_copy_[c & 1]));
        const size_t bytes = (size_t)state_rows_of_block(h, c) * l.row_bytes;
        memcpy(out + off, state_h_[c & 1], bytes);
        off += bytes;
    }
    // the block table last, with the greedy and the feed token in the word behind the checksums
    int *tok = reinterpret_cast<int *>(state_sum_h_ + l.n_blocks);
    if (l.n_blocks) HIP_CHECK(hipMemcpyAsync(state_sum_h_, state_sum_d_, (size_t)8 * l.n_blocks, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(tok, d_argmax_ + slot, 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(tok + 1, d_feed_ + slot, 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    for (uint32_t c = 0; c < l.n_blocks; c++) state_put64(out + l.table + (size_t)8 * c, state_sum_h_[c]);
    auto in_vocab = [&](int t) { return t >= 0 && t < V ? t : 0; };          // (a conversation that never had logits: whatever the words hold is not a token)
    h.greedy = (h.flags & STATE_HAS_LOGITS) ? in_vocab(tok[0]) : 0; h.feed = h.n_rows ? in_vocab(tok[1]) : 0;
    state_write_header(out, h);
    state_info_.saves++; state_info_.rows_saved += h.n_rows;
    return 0;
}
int Engine::state_load(int slot, const void *buf, size_t n) {
    auto fail = [](const std::string &what) { set_last_error("state_load: " + what); return 1; };
    if (slot < 0 || slot >= (int)conv_.size()) return fail("conversation index out of range");
    StateHeader h; StateLayout l; std::string why;
    if (!state_parse(buf, n, h, l, why)) return fail(why);
    if (h.n_layer != layers_.size() || h.n_embd != (uint32_t)llm_.n_embd || h.n_head != (uint32_t)llm_.n_head || h.n_vocab != (uint32_t)llm_.n_vocab)
        return fail("the snapshot's model shape (n_layer " + std::to_string(h.n_layer) + ", n_embd " + std::to_string(h.n_embd) + ", n_head " + std::to_string(h.n_head) + ", n_vocab " +
                    std::to_string(h.n_vocab) + ") is not this context's");
    if (h.arena_hash != llm_arena_.layout_hash) return fail("the snapshot's LLM arena hash is not this context's (another weight file)");
    if (h.n_rows > (uint32_t)n_ctx_) return fail("n_rows " + std::to_string(h.n_rows) + " exceeds n_ctx " + std::to_string(n_ctx_));
    const size_t block_bytes = (size_t)std::min(h.block_rows, std::max(h.n_rows, 1u)) * l.row_bytes;
    if (block_bytes / 16 >= ((size_t)1 << 31)) return fail("a block of " + std::to_string(h.block_rows) + " rows is 2^31 or more 16-byte pieces");
    if (weights_missing()) return fail(last_error());
    state_alloc(block_bytes);                                                // throws before anything changed
    const uint8_t *in = static_cast<const uint8_t *>(buf);
    const int L = (int)h.n_layer, E = (int)h.n_embd, V = (int)h.n_vocab;
    const size_t seq = (size_t)L * n_ctx_ * E;
    // from here on the slot's former content is gone: what reset() does, then the queue
    const SelectScope restore(this);
    cur_ = slot;
    reset();
    Conversation &cv = conv_[(size_t)slot];
    if (logits_host_slot_ == slot) logits_host_slot_ = -1;
    // host memcpy of block c into pinned block i (free once block c - 2's upload is done), upload on the copy stream (device block i is free once block c - 2's
    // unpack is done), unpack on stream_ behind the upload
    size_t off = l.kv;
    for (uint32_t c = 0; c < l.n_blocks; c++) {
        const int i = (int)(c & 1), r0 = (int)(c * h.block_rows), nr = (int)state_rows_of_block(h, c);
        const size_t bytes = (size_t)nr * l.row_bytes;
        if (c >= 2) HIP_CHECK(hipEventSynchronize(state_ev_copy_[i]));
        memcpy(state_h_[i], in + off, bytes);
        off += bytes;
        if (c >= 2) HIP_CHECK(hipStreamWaitEvent(state_cs_, state_ev_kernel_[i], 0));
        HIP_CHECK(hipMemcpyAsync(state_d_[i], state_h_[i], bytes, hipMemcpyHostToDevice, state_cs_));
        HIP_CHECK(hipEventRecord(state_ev_copy_[i], state_cs_));
        HIP_CHECK(hipStreamWaitEvent(stream_, state_ev_copy_[i], 0));
        launch_kv_unpack(state_d_[i], kc_ + (size_t)slot * seq, vc_ + (size_t)slot * seq, n_ctx_, L, E, r0, nr, state_sum_d_ + c, stream_);
        state_info_.unpack_launches++;
        HIP_CHECK(hipEventRecord(state_ev_kernel_[i], stream_));
    }
    if (l.n_blocks) HIP_CHECK(hipMemcpyAsync(state_sum_h_, state_sum_d_, (size_t)8 * l.n_blocks, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));                                // (the copy stream's work lies before stream_'s last unpack)
    for (uint32_t c = 0; c < l.n_blocks; c++)
        if (state_sum_h_[c] != state_get64(in + l.table + (size_t)8 * c)) { state_info_.checksum_failures++; return fail("block " + std::to_string(c) + " checksum"); }
    // everything a following sample, batched step, score, fork, shift or verify pass reads
    const bool has_logits = (h.flags & STATE_HAS_LOGITS) != 0;
    if (has_logits) {
        memcpy(h_logits_, in + l.logits, (size_t)V * 4);                     // through the pinned row: the caller's buffer need not outlive the call
        HIP_CHECK(hipMemcpyAsync(logits_ + (size_t)slot * V, h_logits_, (size_t)V * 4, hipMemcpyHostToDevice, stream_));
    }
    launch_set_int(d_npast_ + slot, (int)h.n_rows, stream_);
    launch_set_int(d_argmax_ + slot, h.greedy, stream_);
    launch_set_int(d_feed_ + slot, h.feed, stream_);
    HIP_CHECK(hipMemcpyAsync(h_argmax_ + slot, d_argmax_ + slot, 4, hipMemcpyDeviceToHost, stream_));   // greedy sample_token reads this copy
    HIP_CHECK(hipStreamSynchronize(stream_));
    logits_host_slot_ = has_logits ? slot : logits_host_slot_;               // h_logits_ holds exactly this row
    cv.n_committed = cv.n_past = (int)h.n_rows;
    cv.hist.resize(h.n_rows);
    for (uint32_t r = 0; r < h.n_rows; r++) cv.hist[r] = (int)state_get32(in + l.hist + (size_t)4 * r);
    cv.has_logits = has_logits;
    const uint8_t *pp = in + l.pen;
    cv.pen.repeat_last_n = (int)state_get32(pp); memcpy(&cv.pen.repeat_penalty, pp + 4, 4); memcpy(&cv.pen.alpha_presence, pp + 8, 4); memcpy(&cv.pen.alpha_frequency, pp + 12, 4);
    cv.pen.penalize_nl = (int)state_get32(pp + 16);
    cv.bias_id.resize(h.n_bias); cv.bias_val.resize(h.n_bias);
    for (uint32_t b = 0; b < h.n_bias; b++) { cv.bias_id[b] = (int)state_get32(in + l.bias + (size_t)8 * b); memcpy(&cv.bias_val[b], in + l.bias + (size_t)8 * b + 4, 4); }
    state_info_.loads++; state_info_.rows_loaded += h.n_rows;
    return 0;
}

// ---- speculation: draft tokens verified in one weight pass (engine.hpp) ----
void Engine::spec_drop_graphs() {
    for (std::vector<hipGraphExec_t> *v : {&spec_graph_, &spec_sgraph_, &mspec_graph_}) for (hipGraphExec_t &g : *v) { if (g) HIP_IGNORE(hipGraphExecDestroy(g)); g = nullptr; }
}
void Engine::spec_free() { spec_drop_graphs(); reset_all(spec_logits_, spec_res_, spec_hres_, sdr_res_, sdr_hres_, mspec_logits_, mspec_res_, mspec_hres_); spec_max_ = 0; }
int Engine::set_speculation(int max_draft) {
    if (max_draft < 0 || max_draft > DRAFT_MAX) { set_last_error("set_speculation: max_draft must be 0 (off) ... " + std::to_string(DRAFT_MAX)); return 1; }
    // the verify pass keeps DRAFT_ROWS new key / value rows next to the score rows in the attention kernel's LDS: a context the one-row form holds may not fit it
    if (const int lim = attn_draft_max_ctx((int)(llm_.n_embd / llm_.n_head)); max_draft > 0 && n_ctx_ > lim) {
        set_last_error("set_speculation: n_ctx " + std::to_string(n_ctx_) + " exceeds what the verify pass's attention kernel holds in LDS at this head size (" + std::to_string(lim) + ")");
        return 1;
    }
    HIP_CHECK(hipStreamSynchronize(stream_));
    spec_free();
    if (max_draft == 0) return 0;
    DevPtr<float> logits((size_t)(max_draft + 1) * llm_.n_vocab * 4); DevPtr<int> res((1 + DRAFT_ROWS) * 4); PinPtr<int> hres((1 + DRAFT_ROWS) * 4);   // all three or none
    spec_logits_ = std::move(logits); spec_res_ = std::move(res); spec_hres_ = std::move(hres);
    spec_graph_.assign((size_t)DRAFT_ROWS + 1, nullptr);
    spec_max_ = max_draft;
    return 0;
}
int Engine::verify_draft(const int *draft, int n_draft, int *ids_out, int *n_out, int *row_greedy, int *n_sent) {
    auto refuse = [](const char *what) { set_last_error(std::string("verify_draft: ") + what); return 1; };
    if (spec_max_ <= 0) return refuse("speculation is off (minigpt4_amd_set_speculation)");
    if (n_draft < 0 || n_draft > spec_max_) return refuse("n_draft outside [0, max_draft]");
    if (n_draft > 0 && !draft) return refuse("draft is NULL");
    if (!ids_out || !n_out) return refuse("ids_out and n_out are required");
    for (int i = 0; i < n_draft; i++) if (draft[i] < 0 || draft[i] >= (int)llm_.n_vocab) return refuse("draft token id out of range");
    if (weights_missing()) return 1;
    Conversation &cv = conv_[(size_t)cur_];
    if (cv.pend_tok.empty() && !cv.has_logits) return refuse("the conversation has no current logits");
    if (flush()) { set_last_error("verify_draft: " + last_error()); return 1; }
    if (!cv.has_logits) return refuse("the conversation has no current logits");
    if (cv.n_past + 1 > n_ctx_ && make_room(1)) return refuse("context full");
    HIP_CHECK(hipStreamSynchronize(stream_));                                // h_argmax_ is current; h_bstage_ no longer feeds an earlier step's copy
    const int g0 = h_argmax_[cur_], p = cv.n_committed;
    const int R = 1 + std::min(n_draft, n_ctx_ - cv.n_past - 1);
    if (n_sent) *n_sent = R - 1;
    if (row_greedy) for (int r = 0; r < 1 + n_draft; r++) row_greedy[r] = -1;   // rows that were not evaluated (cut for room; parity mode: behind the first mismatch)
    int m = 0;
    if (parity_) {   // oracle-order arithmetic exists for the single-row pass only: one row at a time, stopping at the first mismatch -- plain greedy decoding
        for (int r = 0; r < R; r++) {
            const int id = r ? draft[r - 1] : g0;
            if (eval_chunk(&id, 1, nullptr)) return 1;
            cv.n_past += 1;
            HIP_CHECK(hipStreamSynchronize(stream_));
            const int g = h_argmax_[cur_];
            if (row_greedy) row_greedy[r] = g;
            if (r + 1 < R && draft[r] == g) m++; else break;
        }
    } else {
        stage_row(0, g0, cur_, p); for (int r = 1; r < R; r++) staged_token(r) = draft[r - 1];   // k_draft_begin spreads row 0's conversation and position
        step_begin(R, /*verify=*/true);
        step_launch(R, /*verify=*/true);
        HIP_CHECK(hipMemcpyAsync(spec_hres_, spec_res_, (size_t)(1 + R) * 4, hipMemcpyDeviceToHost, stream_));
        HIP_CHECK(hipStreamSynchronize(stream_));                            // the one wait of the call: m and the rows' greedy ids
        m = spec_hres_[0];
        if (m < 0 || m >= R) throw HipError{hipErrorUnknown, "verify_draft: the device reported an accepted count outside the pass", __FILE__, __LINE__};
        if (row_greedy) for (int r = 0; r < R; r++) row_greedy[r] = spec_hres_[1 + r];
        h_argmax_[cur_] = spec_hres_[1 + m];
        commit_rows(cur_, &staged_token(0), 1 + m, /*past=*/true);              // the kept rows only: g0, draft[0 .. m) (the call has synchronised: the slab is whole)
    }
    ids_out[0] = g0; for (int i = 0; i < m; i++) ids_out[1 + i] = draft[i];
    *n_out = 1 + m;
    return 0;
}
int Engine::lookup_check(const char *name, const int *corpus, int n_corpus, int max_tokens, int ngram_max, int ngram_min, int n_draft, const int *tokens_out, const int *n_tokens,
                         const int *stats) const {
    auto refuse = [&](const char *what) { set_last_error(std::string(name) + ": " + what); return 1; };
    if (spec_max_ <= 0) return refuse("speculation is off (minigpt4_amd_set_speculation)");
    if (n_corpus < 0 || (n_corpus > 0 && !corpus)) return refuse("bad corpus");
    if (max_tokens < 1 || !tokens_out || !n_tokens || !stats) return refuse("max_tokens >= 1, tokens_out, n_tokens and stats are required");
    if (ngram_min < 1 || ngram_max < ngram_min) return refuse("need 1 <= ngram_min <= ngram_max");
    if (n_draft < 1 || n_draft > spec_max_) return refuse("n_draft outside [1, max_draft]");
    for (int i = 0; i < n_corpus; i++) if (corpus[i] < 0 || corpus[i] >= (int)llm_.n_vocab) return refuse("corpus token id out of range");
    return 0;
}
int Engine::decode_lookup(const int *corpus, int n_corpus, int max_tokens, int ngram_max, int ngram_min, int n_draft, int *tokens_out, int *n_tokens, int *stats) {
    auto refuse = [](const char *what) { set_last_error(std::string("decode_lookup: ") + what); return 1; };
    if (lookup_check("decode_lookup", corpus, n_corpus, max_tokens, ngram_max, ngram_min, n_draft, tokens_out, n_tokens, stats)) return 1;
    if (weights_missing()) return 1;
    Conversation &cv = conv_[(size_t)cur_];
    if (cv.pend_tok.empty() && !cv.has_logits) return refuse("the conversation has no current logits");
    NgramDrafter drafter(ngram_max, ngram_min);
    drafter.reset(corpus, n_corpus);
    int n = 0, st[4] = {0, 0, 0, 0}, d[DRAFT_MAX], ids[DRAFT_ROWS];
    *n_tokens = 0;
    auto done = [&](int rc) { *n_tokens = n; for (int i = 0; i < 4; i++) stats[i] = st[i]; return rc; };
    while (n < max_tokens) {
        const int g0 = greedy_raw();                                        // evaluates what is queued; the token the next pass evaluates (raw logits: no penalties here)
        if (cv.n_past + 1 > n_ctx_ && make_room(1)) break;                   // context full and no automatic shift
        drafter.push(g0);
        const int nd = g0 == 2 ? 0 : drafter.draft(std::min(n_draft, max_tokens - n - 1), d);
        if (nd == 0) {                                                       // nothing to guess from: the ordinary decode step, at its ordinary cost
            if (add_tokens({g0}, /*flush_now=*/true)) { set_last_error("decode_lookup: " + last_error()); return done(1); }
            tokens_out[n++] = g0; st[1]++;
        } else {
            int got = 0, sent = 0;
            if (verify_draft(d, nd, ids, &got, nullptr, &sent)) { set_last_error("decode_lookup: " + last_error()); return done(1); }
            st[0]++; st[2] += sent; st[3] += got - 1;
            for (int i = 0; i < got; i++) { tokens_out[n++] = ids[i]; if (i) drafter.push(ids[i]); }
        }
        if (g0 == 2) break;                                                  // </s> emitted and evaluated
    }
    return done(0);
}
// ---- speculation, greedy, several conversations in one weight pass (engine.hpp) ----
void Engine::mspec_alloc() {
    if (mspec_graph_.empty()) mspec_graph_.assign((size_t)ATTN_MDRAFT_ROWS + 1, nullptr);
    if (mspec_logits_) return;
    DevPtr<float> logits((size_t)ATTN_MDRAFT_ROWS * llm_.n_vocab * 4); DevPtr<int> res(2 * ATTN_MDRAFT_ROWS * 4); PinPtr<int> hres(2 * ATTN_MDRAFT_ROWS * 4);   // all three or none
    mspec_logits_ = std::move(logits); mspec_res_ = std::move(res); mspec_hres_ = std::move(hres);
}
int Engine::speculation_batch_info(long long out[8]) const {
    if (!out) { set_last_error("speculation_batch_info: no output array"); return 1; }
    const SpecBatchInfo &i = mspec_info_;
    out[0] = i.passes; out[1] = i.rows; out[2] = i.groups; out[3] = i.sent; out[4] = i.accepted; out[5] = i.plain; out[6] = i.cut; out[7] = 0;
    return 0;
}
int Engine::verify_draft_batch(const int *slots, int n, const int *drafts, const int *counts, int *ids_out, int *n_out, int *row_greedy) {
    auto refuse = [](const std::string &what) { set_last_error("verify_draft_batch: " + what); return 1; };
    if (spec_max_ <= 0) return refuse("speculation is off (minigpt4_amd_set_speculation)");
    if (const int bad = check_slots(slots, n)) return refuse(bad == 1 ? "bad slot list" : "conversations must be distinct and in range");
    if (!counts || !ids_out || !n_out) return refuse("counts, ids_out and n_out are required");
    int n_drafts = 0;
    for (int i = 0; i < n; i++) { if (counts[i] < 0 || counts[i] > spec_max_) return refuse("a count outside [0, max_draft]"); n_drafts += counts[i]; }
    if (n_drafts > 0 && !drafts) return refuse("drafts is NULL");
    for (int i = 0; i < n_drafts; i++) if (drafts[i] < 0 || drafts[i] >= (int)llm_.n_vocab) return refuse("draft token id out of range");
    const int row_cap = std::min(ATTN_MDRAFT_ROWS, max_rows_);
    if (n + n_drafts > row_cap) return refuse("more rows in total (" + std::to_string(n + n_drafts) + ") than the pass holds (" + std::to_string(row_cap) + ")");
    if (weights_missing()) return 1;
    for (int i = 0; i < n; i++) { const Conversation &cv = conv_[(size_t)slots[i]]; if (cv.pend_tok.empty() && !cv.has_logits) return refuse("a conversation has no current logits"); }
    const SelectScope restore(this);
    for (int i = 0; i < n; i++) {                                             // queued prompt rows of each conversation first, as decode_batch does
        cur_ = slots[i];
        if (flush()) return refuse(last_error());
        if (!conv_[(size_t)cur_].has_logits) return refuse("a conversation has no current logits");
    }
    if (row_greedy) std::fill(row_greedy, row_greedy + (size_t)n * DRAFT_ROWS, -1);   // rows that were not evaluated
    // the rows each conversation brings: 0 = no room (and no automatic shift), left out; a draft is cut to the room left
    int R[MAX_CONVERSATIONS], off[MAX_CONVERSATIONS], N = 0, G = 0, cut = 0; bool any_draft = false;
    for (int i = 0, o = 0; i < n; o += counts[i], i++) {
        Conversation &cv = conv_[(size_t)slots[i]];
        cur_ = slots[i]; off[i] = o; n_out[i] = 0;
        if (cv.n_past + 1 > n_ctx_ && make_room(1)) { R[i] = 0; continue; }
        R[i] = 1 + std::min(counts[i], n_ctx_ - cv.n_past - 1);
        cut += counts[i] - (R[i] - 1); N += R[i]; G++; any_draft = any_draft || R[i] > 1;
    }
    mspec_info_.cut += cut;
    if (!G) return 0;
    if (parity_) {   // oracle-order arithmetic exists for the single-row pass only: verify_draft's one-row loop per conversation -- plain greedy decoding
        for (int i = 0; i < n; i++) {
            if (!R[i]) continue;
            cur_ = slots[i];
            int rg[DRAFT_ROWS];
            if (verify_draft(drafts + off[i], counts[i], ids_out + (size_t)i * DRAFT_ROWS, &n_out[i], rg)) return refuse(last_error());
            if (row_greedy) std::copy(rg, rg + 1 + counts[i], row_greedy + (size_t)i * DRAFT_ROWS);
        }
        return 0;
    }
    HIP_CHECK(hipStreamSynchronize(stream_));                                // h_argmax_ is current; h_bstage_ no longer feeds an earlier step's copy
    if (!any_draft) {                                                        // nothing to verify: the ordinary batched step, its own graph and k_batch_finish
        int B = 0;
        for (int i = 0; i < n; i++) if (R[i]) { ids_out[(size_t)i * DRAFT_ROWS] = h_argmax_[slots[i]]; stage_row(B++, h_argmax_[slots[i]], slots[i], conv_[(size_t)slots[i]].n_committed); }
        step_begin(B);
        step_launch(B);
        for (int r = 0; r < B; r++) commit_rows(staged_slot(r), &staged_token(r), 1, /*past=*/true);
        HIP_CHECK(hipMemcpyAsync(h_argmax_, d_argmax_, conv_.size() * 4, hipMemcpyDeviceToHost, stream_));
        for (int i = 0; i < n; i++) if (R[i]) n_out[i] = 1;
        if (row_greedy) {
            HIP_CHECK(hipStreamSynchronize(stream_));
            for (int i = 0; i < n; i++) if (R[i]) row_greedy[(size_t)i * DRAFT_ROWS] = h_argmax_[slots[i]];
        }
        mspec_info_.plain++;
        return 0;
    }
    mspec_alloc();
    int t0[MAX_CONVERSATIONS];
    for (int i = 0, t = 0; i < n; i++) {
        if (!R[i]) continue;
        const int p = conv_[(size_t)slots[i]].n_committed;
        t0[i] = t;
        stage_row(t, h_argmax_[slots[i]], slots[i], p);
        for (int r = 1; r < R[i]; r++) stage_row(t + r, drafts[off[i] + r - 1], slots[i], p + r);
        t += R[i];
    }
    step_begin(N, /*verify=*/false, /*multi=*/true);
    step_launch(N, /*verify=*/false, /*epilogue=*/true, /*multi=*/true);
    HIP_CHECK(hipMemcpyAsync(mspec_hres_, mspec_res_, 2 * ATTN_MDRAFT_ROWS * 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));                                // the one wait of the pass: every group's m and the rows' greedy ids
    const int *hm = mspec_hres_, *hg = hm + ATTN_MDRAFT_ROWS;
    for (int i = 0; i < n; i++) if (R[i] && (hm[t0[i]] < 0 || hm[t0[i]] >= R[i]))
        throw HipError{hipErrorUnknown, "verify_draft_batch: the device reported an accepted count outside a group", __FILE__, __LINE__};
    long long acc = 0;
    for (int i = 0; i < n; i++) {
        if (!R[i]) continue;
        const int m = hm[t0[i]], slot = slots[i];
        if (row_greedy) for (int r = 0; r < R[i]; r++) row_greedy[(size_t)i * DRAFT_ROWS + r] = hg[t0[i] + r];
        h_argmax_[slot] = hg[t0[i] + m];
        commit_rows(slot, &staged_token(t0[i]), 1 + m, /*past=*/true);         // the kept rows only: g0, draft[0 .. m)
        for (int r = 0; r <= m; r++) ids_out[(size_t)i * DRAFT_ROWS + r] = staged_token(t0[i] + r);
        n_out[i] = 1 + m; acc += m;
    }
    mspec_info_.passes++; mspec_info_.rows += N; mspec_info_.groups += G; mspec_info_.sent += N - G; mspec_info_.accepted += acc;
    return 0;
}
int Engine::decode_lookup_batch(const int *slots, int n, const int *corpus, const int *corpus_counts, int max_tokens, int ngram_max, int ngram_min, int n_draft, int *tokens_out,
                                int *n_tokens, int *stats) {
    auto refuse = [](const std::string &what) { set_last_error("decode_lookup_batch: " + what); return 1; };
    if (const int bad = check_slots(slots, n)) return refuse(bad == 1 ? "bad slot list" : "conversations must be distinct and in range");
    if (!corpus_counts) return refuse("corpus_counts is NULL");
    int n_corpus = 0;
    for (int i = 0; i < n; i++) { if (corpus_counts[i] < 0) return refuse("bad corpus"); n_corpus += corpus_counts[i]; }
    if (lookup_check("decode_lookup_batch", corpus, n_corpus, max_tokens, ngram_max, ngram_min, n_draft, tokens_out, n_tokens, stats)) return 1;
    if (weights_missing()) return 1;
    for (int i = 0; i < n; i++) { const Conversation &cv = conv_[(size_t)slots[i]]; if (cv.pend_tok.empty() && !cv.has_logits) return refuse("a conversation has no current logits"); }
    std::vector<NgramDrafter> drafter((size_t)n, NgramDrafter(ngram_max, ngram_min));
    for (int i = 0, o = 0; i < n; o += corpus_counts[i], i++) drafter[(size_t)i].reset(corpus + o, corpus_counts[i]);
    std::vector<char> running((size_t)n, 1);
    std::fill(n_tokens, n_tokens + n, 0); std::fill(stats, stats + (size_t)4 * n, 0);
    const SelectScope restore(this);
    const int row_cap = std::min(ATTN_MDRAFT_ROWS, max_rows_);
    int who[MAX_CONVERSATIONS], sl[MAX_CONVERSATIONS], cnt[MAX_CONVERSATIONS], g0s[MAX_CONVERSATIONS], got[MAX_CONVERSATIONS];
    std::vector<int> d((size_t)n * DRAFT_MAX), ids((size_t)n * DRAFT_ROWS);
    for (;;) {
        int k = 0, nd_all = 0, live = 0;
        for (int i = 0; i < n; i++) live += running[(size_t)i];
        int spare = row_cap - live;                                          // draft rows the pass still holds beside one row per running conversation
        for (int i = 0; i < n; i++) {
            if (!running[(size_t)i]) continue;
            Conversation &cv = conv_[(size_t)slots[i]];
            cur_ = slots[i];
            const int g0 = greedy_raw();                                     // evaluates what is queued; raw logits: no penalties here
            if (cv.n_past + 1 > n_ctx_ && make_room(1)) { running[(size_t)i] = 0; continue; }   // context full and no automatic shift
            drafter[(size_t)i].push(g0);
            const int want = std::min(std::min(n_draft, max_tokens - n_tokens[i] - 1), std::min(n_ctx_ - cv.n_past - 1, spare));
            const int nd = g0 == 2 || want <= 0 ? 0 : drafter[(size_t)i].draft(want, d.data() + nd_all);
            who[k] = i; sl[k] = slots[i]; cnt[k] = nd; g0s[k] = g0; k++; nd_all += nd; spare -= nd;
        }
        if (!k) break;
        if (verify_draft_batch(sl, k, d.data(), cnt, ids.data(), got, nullptr)) return refuse(last_error());
        for (int j = 0; j < k; j++) {
            const int i = who[j];
            if (got[j] < 1) { running[(size_t)i] = 0; continue; }
            stats[4 * i + (cnt[j] ? 0 : 1)]++; stats[4 * i + 2] += cnt[j]; stats[4 * i + 3] += got[j] - 1;
            for (int r = 0; r < got[j]; r++) { const int id = ids[(size_t)j * DRAFT_ROWS + r]; tokens_out[(size_t)i * max_tokens + n_tokens[i]++] = id; if (r) drafter[(size_t)i].push(id); }
            if (g0s[j] == 2 || n_tokens[i] >= max_tokens) running[(size_t)i] = 0;   // </s> emitted and evaluated, or the budget spent
        }
    }
    return 0;
}
// ---- speculation under sampling (engine.hpp, draft_host.hpp) ----
void Engine::sdr_alloc() {
    if (spec_sgraph_.empty()) spec_sgraph_.assign((size_t)DRAFT_ROWS + 1, nullptr);
    if (sdr_res_) return;
    DevPtr<int> d(DRAFT_SAMPLE_RES * 4); PinPtr<int> h(DRAFT_SAMPLE_RES * 4);   // both or none
    sdr_res_ = std::move(d); sdr_hres_ = std::move(h);
}
int Engine::speculation_info(long long out[8]) const {
    if (!out) { set_last_error("speculation_info: no output array"); return 1; }
    const SpecInfo &i = spec_info_;
    out[0] = i.passes; out[1] = i.rows; out[2] = i.sent; out[3] = i.accepted; out[4] = i.launches; out[5] = i.stuck; out[6] = i.cut; out[7] = 0;
    return 0;
}
int Engine::verify_draft_sampled(const int *draft, int n_draft, float temp, int top_k, float top_p, int *ids_out, int *n_out, int *next_out, int *row_sampled, float *row_logits,
                                 const char *name, int *n_sent) {
    return verify_draft_sampled_t<false>(draft, n_draft, temp, top_k, top_p, nullptr, ids_out, n_out, next_out, row_sampled, row_logits, name, n_sent);
}
int Engine::verify_draft_sampled_ex(const int *draft, int n_draft, float temp, int top_k, float top_p, const ChainParams &cp, int *ids_out, int *n_out, int *next_out, int *row_sampled,
                                    float *row_logits) {
    return verify_draft_sampled_t<true>(draft, n_draft, temp, top_k, top_p, &cp, ids_out, n_out, next_out, row_sampled, row_logits, "verify_draft_sampled_ex", nullptr);
}
template <bool EX> int Engine::verify_draft_sampled_t(const int *draft, int n_draft, float temp, int top_k, float top_p, const ChainParams *cp, int *ids_out, int *n_out, int *next_out,
                                                      int *row_sampled, float *row_logits, const char *name, int *n_sent) {
    auto refuse = [&](const std::string &what) { set_last_error(std::string(name) + ": " + what); return 1; };
    const int V = (int)llm_.n_vocab;
    if (spec_max_ <= 0) return refuse("speculation is off (minigpt4_amd_set_speculation)");
    if (n_draft < 0 || n_draft > spec_max_) return refuse("n_draft outside [0, max_draft]");
    if (n_draft > 0 && !draft) return refuse("draft is NULL");
    if (!ids_out || !n_out || !next_out) return refuse("ids_out, n_out and next_out are required");
    for (int i = 0; i < n_draft; i++) if (draft[i] < 0 || draft[i] >= V) return refuse("draft token id out of range");
    if (!sampling_params_ok(refuse, temp, top_k, top_p)) return 1;
    if (cp && !chain_params_ok(refuse, *cp)) return 1;
    if (weights_missing()) return refuse(last_error());
    Conversation &cv = conv_[(size_t)cur_];
    if (cv.pend_tok.empty() && !cv.has_logits) return refuse("the conversation has no current logits");
    if (flush()) return refuse("the queued rows could not be evaluated: " + last_error());
    if (!cv.has_logits) return refuse("the conversation has no current logits");
    if (cv.n_past + 1 > n_ctx_ && !shift_allows(1)) return refuse("context full");   // before anything is decided: no draw is counted for a call that cannot emit
    HIP_CHECK(hipStreamSynchronize(stream_));                                // the history is whole; h_bstage_ and smp_ feed no earlier copy
    const int slot = cur_, handle = con_handle_[slot];
    const uint64_t c0 = smp_draws_[slot];
    sdr_alloc();
    auto &blk = smp_block<EX>();
    constexpr const char *refused = EX ? "verify_draft_sampled_ex: a launch was refused (minigpt4_amd_last_error)" : "verify_draft_sampled: a launch was refused (minigpt4_amd_last_error)";
    constexpr const char *bad_pick = EX ? "verify_draft_sampled_ex: the device reported an id outside the vocabulary" : "verify_draft_sampled: the device reported an id outside the vocabulary";
    // 1. x0 = D(L, h, q, c): the sampled step's own descriptor (history before the shift) and launch, on the conversation's row; the host needs the pick for the rows' tables
    const size_t n_ent0 = smp_stage<EX>(&slot, 1, temp, top_k, top_p, cp);
    if (cv.n_past + 1 > n_ctx_ && make_room(1)) return refuse("context full");
    auto decide = [&](size_t n_ent, int *stuck) -> int {                     // the staged descriptor on logits_, the 8 bytes {pick, stuck} awaited
        if (!smp_launch_on<EX>(logits_, 1, n_ent)) throw HipError{hipErrorInvalidValue, refused, __FILE__, __LINE__};
        blk.fetch(1, 2 * sizeof(int), stream_);
        HIP_CHECK(hipStreamSynchronize(stream_));
        spec_info_.launches++;
        const int id = device_id(smp_plain(blk.out_h()[0]).pick, bad_pick);
        *stuck = smp_plain(blk.out_h()[0]).stuck == 1;
        return id;
    };
    int stuck0 = 0;
    const int x0 = decide(n_ent0, &stuck0), p = cv.n_committed;
    spec_info_.stuck += stuck0;
    // 2. the rows: the draft cut to the room left, then at the first token its constraint state does not allow; one table and one state per row
    const int room = std::min(n_draft, n_ctx_ - cv.n_past - 1);
    const PenParams pp = pen_mode_ ? cv.pen : PenParams{};
    auto piece = [&](int id, const unsigned char **b, int *n) {
        if (id < 0 || id >= (int)llm_.pieces.size()) return false;
        *b = reinterpret_cast<const unsigned char *>(llm_.pieces[(size_t)id].data()); *n = (int)llm_.pieces[(size_t)id].size();
        return true;
    };
    DraftStage st;
    draft_stage(cv.hist.data(), cv.hist.size(), x0, draft, room, pp, cv.bias_id.data(), cv.bias_val.data(), (int)cv.bias_id.size(), n_ctx_, V,
                handle ? &con_[handle - 1].dfa : nullptr, con_state_[slot], piece, st);
    const int R = st.n_rows;
    if (n_sent) *n_sent = R - 1;
    if (row_sampled) for (int r = 0; r < 1 + n_draft; r++) row_sampled[r] = -1;   // rows that were not evaluated (cut; parity mode: behind the first mismatch)
    spec_info_.passes++; spec_info_.sent += R - 1; spec_info_.cut += st.cut;
    int m = 0, next = -1;
    if (parity_) {   // oracle-order arithmetic exists for the single-row pass only: evaluate a row, decide on the conversation's own row, stop at the first mismatch
        smp_draws_[slot] = c0 + 1; if (handle) con_walk(slot, x0);
        for (int r = 0; r < R; r++) {
            const int id = r ? draft[r - 1] : x0;
            if (eval_chunk(&id, 1, nullptr)) return 1;
            cv.n_past += 1;
            HIP_CHECK(hipStreamSynchronize(stream_));
            spec_info_.rows++;
            if (row_logits) { HIP_CHECK(hipMemcpyAsync(row_logits + (size_t)r * V, logits_ + (size_t)slot * V, (size_t)V * 4, hipMemcpyDeviceToHost, stream_)); HIP_CHECK(hipStreamSynchronize(stream_)); }
            int stuck = 0;
            const int x = decide(smp_stage<EX>(&slot, 1, temp, top_k, top_p, cp), &stuck);   // history h_r, state q_r, draw c + 1 + r: all current
            spec_info_.stuck += stuck;
            if (row_sampled) row_sampled[r] = x;
            next = x;
            if (r + 1 < R && draft[r] == x) { m++; smp_draws_[slot] += 1; if (handle) con_walk(slot, x); } else break;
        }
    } else {
        // 3. behind one wait: the slab, the pass without an epilogue, the R decisions with draws c + 1 + r, the epilogue, the result block
        for (int r = 0; r < R; r++) {
            smp_plain(blk.rows()[r]) = smp_row(slot, st.rows[(size_t)r], st.state[(size_t)r], c0 + 1 + (uint64_t)r, -1, temp, top_k, top_p);
            if constexpr (EX) blk.rows()[r].chain = *cp;
        }
        std::copy(st.entries.begin(), st.entries.end(), blk.entries());
        stage_row(0, x0, slot, p); for (int r = 1; r < R; r++) staged_token(r) = draft[r - 1];   // k_draft_begin spreads row 0's conversation and position
        step_begin(R, /*verify=*/true);
        step_launch(R, /*verify=*/true, /*epilogue=*/false);
        if (!smp_launch_on<EX>(spec_logits_, R, st.entries.size())) throw HipError{hipErrorInvalidValue, refused, __FILE__, __LINE__};
        if (!launch_draft_sample_finish(spec_logits_, V, V, R, d_btok_, blk.out_d(), d_bslot_, d_npast_, d_argmax_, d_feed_, logits_, sdr_res_, stream_))
            throw HipError{hipErrorInvalidValue, refused, __FILE__, __LINE__};
        spec_info_.launches++; spec_info_.rows += R;
        HIP_CHECK(hipMemcpyAsync(sdr_hres_, sdr_res_, DRAFT_SAMPLE_RES * 4, hipMemcpyDeviceToHost, stream_));
        HIP_CHECK(hipMemcpyAsync(h_argmax_, d_argmax_, conv_.size() * 4, hipMemcpyDeviceToHost, stream_));
        if (row_logits) HIP_CHECK(hipMemcpyAsync(row_logits, spec_logits_, (size_t)R * V * 4, hipMemcpyDeviceToHost, stream_));
        HIP_CHECK(hipStreamSynchronize(stream_));                            // the one wait behind the pass: m, the rows' samples, their stuck flags
        m = sdr_hres_[0];
        // the device has advanced the conversation by 1 + m whatever the block says: the book-keeping follows it before a bad block is reported
        const bool sane = m >= 0 && m < R;
        if (!sane) m = 0;
        commit_rows(slot, &staged_token(0), 1 + m, /*past=*/true);              // the kept rows only: x0, draft[0 .. m)
        smp_draws_[slot] = c0 + 1 + (uint64_t)m;
        if (handle) con_state_[slot] = st.state[(size_t)m];
        if (!sane) throw HipError{hipErrorUnknown, EX ? "verify_draft_sampled_ex: the device reported an accepted count outside the pass" : "verify_draft_sampled: the device reported an accepted count outside the pass", __FILE__, __LINE__};
        for (int r = 0; r < R; r++) { if (row_sampled) row_sampled[r] = sdr_hres_[1 + r]; spec_info_.stuck += sdr_hres_[1 + DRAFT_ROWS + r] == 1; }
        next = sdr_hres_[1 + m];
        device_id(next, bad_pick);
    }
    spec_info_.accepted += m;
    ids_out[0] = x0; for (int i = 0; i < m; i++) ids_out[1 + i] = draft[i];
    *n_out = 1 + m; *next_out = next;
    return 0;
}
int Engine::decode_lookup_sampled(const int *corpus, int n_corpus, int max_tokens, int ngram_max, int ngram_min, int n_draft, float temp, int top_k, float top_p, int *tokens_out,
                                  int *n_tokens, int *stats) {
    return decode_lookup_sampled_t<false>(corpus, n_corpus, max_tokens, ngram_max, ngram_min, n_draft, temp, top_k, top_p, nullptr, tokens_out, n_tokens, stats);
}
int Engine::decode_lookup_sampled_ex(const int *corpus, int n_corpus, int max_tokens, int ngram_max, int ngram_min, int n_draft, float temp, int top_k, float top_p, const ChainParams &cp,
                                     int *tokens_out, int *n_tokens, int *stats) {
    return decode_lookup_sampled_t<true>(corpus, n_corpus, max_tokens, ngram_max, ngram_min, n_draft, temp, top_k, top_p, &cp, tokens_out, n_tokens, stats);
}
template <bool EX> int Engine::decode_lookup_sampled_t(const int *corpus, int n_corpus, int max_tokens, int ngram_max, int ngram_min, int n_draft, float temp, int top_k, float top_p,
                                                       const ChainParams *cp, int *tokens_out, int *n_tokens, int *stats) {
    static const char *const name = EX ? "decode_lookup_sampled_ex" : "decode_lookup_sampled";
    auto refuse = [](const char *what) { set_last_error(std::string(name) + ": " + what); return 1; };
    if (lookup_check(name, corpus, n_corpus, max_tokens, ngram_max, ngram_min, n_draft, tokens_out, n_tokens, stats)) return 1;
    if (!sampling_params_ok(refuse, temp, top_k, top_p)) return 1;
    if (cp && !chain_params_ok(refuse, *cp)) return 1;
    if (weights_missing()) return 1;
    Conversation &cv = conv_[(size_t)cur_];
    if (cv.pend_tok.empty() && !cv.has_logits) return refuse("the conversation has no current logits");
    NgramDrafter drafter(ngram_max, ngram_min);
    drafter.reset(corpus, n_corpus);
    int n = 0, st[4] = {0, 0, 0, 0}, d[DRAFT_MAX], ids[DRAFT_ROWS], next = -1;
    *n_tokens = 0;
    auto done = [&](int rc) { *n_tokens = n; for (int i = 0; i < 4; i++) stats[i] = st[i]; return rc; };
    while (n < max_tokens) {
        if (cv.n_past + 1 > n_ctx_ && !shift_allows(1)) break;               // context full and no automatic shift (n_past counts the queued rows)
        // the draft continues the history behind `next`, the token the coming pass evaluates first (unknown before the first pass: that one runs without a draft)
        const int announced = next;
        int nd = 0;
        if (announced >= 0 && announced != 2) {
            drafter.push(announced);
            nd = drafter.draft(std::min(n_draft, max_tokens - n - 1), d);
        }
        int got = 0, sent = 0;
        if (verify_draft_sampled_t<EX>(d, nd, temp, top_k, top_p, cp, ids, &got, &next, nullptr, nullptr, name, &sent)) return done(1);
        // x0 is the announced token wherever the logits are the same; in fast mode a pass of another shape may have rounded a logit differently and moved the draw across a
        // boundary: the history takes what was emitted (the draft then missed: m = 0 or a lucky match, both within the rule)
        if (announced < 0 || announced == 2) drafter.push(ids[0]);
        else if (ids[0] != announced) { drafter.reset(corpus, n_corpus); for (int i = 0; i < n; i++) drafter.push(tokens_out[i]); drafter.push(ids[0]); }
        if (nd) { st[0]++; st[2] += sent; st[3] += got - 1; } else st[1]++;
        for (int i = 0; i < got; i++) { tokens_out[n++] = ids[i]; if (i) drafter.push(ids[i]); }
        if (ids[0] == 2) break;                                              // </s> emitted and evaluated (a draft never holds it)
    }
    return done(0);
}

// The segmented prompt attention of one packed chunk: one launch over every segment; when it declines (the exact-f32 kernel is selected, or the score
// rows do not fit LDS), one launch of the single-conversation kernels per segment, with its rows, its cache and its position.
void Engine::attn_segments(const SegChunk &sg, __half *kc, __half *vc, bool want_h, bool *att_in_xh, hipStream_t s) {
    const int E = (int)llm_.n_embd, H = (int)llm_.n_head, hd = E / H;
    if (attn_prefill_ && launch_attn_prefill_seg(q_, kc, vc, sg.att, H, hd, tabs_, att_, tune_, s, want_h ? act_.xh : nullptr, att_in_xh)) return;
    *att_in_xh = false;
    const size_t seq_stride = layers_.size() * (size_t)n_ctx_ * E;
    for (int i = 0; i < sg.n_seg; i++) {
        const int *g = sg.h_segs + 4 * i;
        const size_t off = (size_t)g[1] * E, cs = (size_t)g[0] * seq_stride;
        const int *np = sg.att.segs + 4 * i + 3;                            // the segment's first position, in device memory
        if (!(attn_prefill_ && launch_attn_prefill(q_ + off, kc + cs, vc + cs, g[2], H, hd, np, g[3] + g[2], tabs_, att_ + off, tune_, s)))
            launch_attn_llm(q_ + off, k_ + off, v_ + off, kc + cs, vc + cs, g[2], H, hd, np, n_ctx_, cos_, sin_, tabs_, att_ + off, false, s);
    }
}

// Queued prompt rows of several conversations in one pass over the weights per chunk.  Rows do not depend on each other in the mat-muls (activations are
// quantised per row), so the conversations' rows are packed like flush() packs one conversation's fragments; RoPE + cache append, the attention and the
// output rows learn each row's conversation from the chunk's tables.  A conversation may continue in the next chunk at its advanced position.
int Engine::prefill_batch(const int *slots, int n) {
    if (const int bad = check_slots(slots, n)) { set_last_error(bad == 1 ? "prefill_batch: bad slot list" : "prefill_batch: conversations must be distinct and in range"); return 1; }
    if (weights_missing()) return 1;
    const SelectScope restore(this);
    try {
        // oracle-order arithmetic (parity mode) and the parity trace exist for the single-conversation pass only: one flush per conversation, in slot order
        if (parity_ || trace_file_) {
            int reused = 0;                                                  // rows_last of the call = the sum over its conversations, as in the packed form
            for (int i = 0; i < n; i++) { cur_ = slots[i]; pfx_.rows_last = 0; if (flush()) { drop_queues(slots, n); return 1; } reused += pfx_.rows_last; }
            if (pfx_max_ > 0) pfx_.rows_last = reused;
            return 0;
        }
        if (prefill_packed(slots, n)) { drop_queues(slots, n); return 1; }
    } catch (...) { drop_queues(slots, n); throw; }
    return 0;
}
int Engine::prefill_packed(const int *slots, int n, const ScoreOut *so) {
    const int E = (int)llm_.n_embd;
    // prefix store (engine.hpp): a conversation the store serves starts at queue row m, its segments at pos0 = m.  A score pass neither consults nor captures the store: a
    // copied row has no logits
    const PrefixPlan plan = so ? PrefixPlan{} : prefix_lookup(slots, n);
    struct Src { int slot; size_t row, erow; };                              // next queued row / embedding row of a conversation
    std::vector<Src> src;
    for (int i = 0; i < n; i++) if (!conv_[(size_t)slots[i]].pend_tok.empty()) src.push_back({slots[i], (size_t)plan.m[i], 0});
    if (src.empty()) return 0;
    std::vector<int> tok, tgt, dest, h_gr; std::vector<float> h_lp, h_glp;   // score pass: per packed row, the id it predicts (-1: none) and the output entry that takes its result
    size_t k = 0;
    while (k < src.size()) {
        HIP_CHECK(hipStreamSynchronize(stream_));                            // h_seg_ may still feed the previous chunk's copy
        SegChunk sc;
        int *const hs = h_seg_, *const fin = hs + SEG_FIN, *const last = hs + SEG_LAST, *const rows = hs + SEG_ROWS;
        int *const t16 = rows + 2 * (size_t)max_rows_, *const t32 = t16 + 2 * ((size_t)max_rows_ + MAX_CONVERSATIONS);
        int N = 0;
        tok.clear(); tgt.clear(); dest.clear();
        while (k < src.size() && N < max_chunk_) {
            Src &c = src[k];
            Conversation &cv = conv_[(size_t)c.slot];
            const int m = (int)std::min((size_t)(max_chunk_ - N), cv.pend_tok.size() - c.row), pos0 = cv.n_committed;
            int *g = hs + 4 * sc.n_seg;
            g[0] = c.slot; g[1] = N; g[2] = m; g[3] = pos0;
            sc.key_rows += (double)(pos0 + m);
            sc.att.t_max = std::max(sc.att.t_max, pos0 + m);
            for (int r = 0; r < m; r++) { rows[2 * (N + r)] = c.slot; rows[2 * (N + r) + 1] = pos0 + r; tok.push_back(cv.pend_tok[c.row + r]); }
            if (so) for (int r = 0; r < m; r++) {   // the queue holds exactly the call's tokens: row j predicts token j + 1, the conversation's last row nothing
                const size_t nx = c.row + (size_t)r + 1;
                const bool has = nx < cv.pend_tok.size();
                tgt.push_back(has ? cv.pend_tok[nx] : -1); dest.push_back(has ? so->off[c.slot] + (int)nx : -1);
            }
            c.erow += upload_embd_runs(cv.pend_tok.data() + c.row, m, cv.pend_embd.data() + c.erow * E, x_ + (size_t)N * E);   // at their packed rows
            c.row += (size_t)m;
            if (c.row == cv.pend_tok.size()) { fin[2 * sc.n_end] = c.slot; fin[2 * sc.n_end + 1] = pos0 + m; last[sc.n_end] = N + m - 1; sc.n_end++; k++; }
            if (logits_host_slot_ == c.slot) logits_host_slot_ = -1;
            N += m; sc.n_seg++;
        }
        memcpy(sc.h_segs, hs, (size_t)sc.n_seg * 4 * sizeof(int));
        sc.att.n_tiles[0] = attn_seg_tiles(hs, sc.n_seg, 16, t16);
        sc.att.n_tiles[1] = attn_seg_tiles(hs, sc.n_seg, 32, t32);
        sc.att.segs = d_seg_; sc.att.tiles[0] = d_seg_ + (t16 - hs); sc.att.tiles[1] = d_seg_ + (t32 - hs);
        sc.att.seq_stride = layers_.size() * (size_t)n_ctx_ * E;
        sc.rows = d_seg_ + SEG_ROWS; sc.fin = d_seg_ + SEG_FIN; sc.last = d_seg_ + SEG_LAST;
        HIP_CHECK(hipMemcpyAsync(d_seg_, h_seg_, seg_ints() * 4, hipMemcpyHostToDevice, stream_));
        HIP_CHECK(hipMemcpyAsync(d_tokens_, tok.data(), (size_t)N * 4, hipMemcpyHostToDevice, stream_));
        HIP_CHECK(hipStreamSynchronize(stream_));                            // the (pageable) queues may be changed right after this call
        const ScoreReq rq = so ? score_request(tgt, 0, nullptr) : ScoreReq{};
        Pass p{N}; p.seg = &sc;
        if (rq.end > rq.first) p.score = &rq;                               // (a chunk without a target row runs exactly as prefill_batch runs it)
        forward(p, stream_);                                                 // k_get_rows skips rows whose id is negative
        if (p.score) {
            const size_t nr = (size_t)(rq.end - rq.first);
            h_lp.resize(nr); h_glp.resize(nr); h_gr.resize(nr);
            HIP_CHECK(hipMemcpyAsync(h_lp.data(), score_lp_ + rq.first, nr * 4, hipMemcpyDeviceToHost, stream_));
            HIP_CHECK(hipMemcpyAsync(h_glp.data(), score_glp_ + rq.first, nr * 4, hipMemcpyDeviceToHost, stream_));
            HIP_CHECK(hipMemcpyAsync(h_gr.data(), score_greedy_ + rq.first, nr * 4, hipMemcpyDeviceToHost, stream_));
            HIP_CHECK(hipStreamSynchronize(stream_));
            for (int r = rq.first; r < rq.end; r++) {
                const int d = dest[(size_t)r];
                if (d < 0) continue;
                so->logprob[d] = h_lp[(size_t)(r - rq.first)];
                if (so->greedy) so->greedy[d] = h_gr[(size_t)(r - rq.first)];
                if (so->greedy_logprob) so->greedy_logprob[d] = h_glp[(size_t)(r - rq.first)];
            }
        }
        for (int i = 0; i < sc.n_seg; i++) {
            const int *g = sc.h_segs + 4 * i;
            Conversation &cv = conv_[(size_t)g[0]];
            // (not commit_rows: a segment that continues in the next chunk has no logits row yet -- has_logits waits for the last chunk, below)
            cv.n_committed += g[2]; cv.hist.insert(cv.hist.end(), tok.begin() + g[1], tok.begin() + g[1] + g[2]);
        }
    }
    for (const Src &c : src) { Conversation &cv = conv_[(size_t)c.slot]; cv.drop_queue(); cv.has_logits = true; }
    prefix_commit(plan);
    HIP_CHECK(hipMemcpyAsync(h_argmax_, d_argmax_, conv_.size() * 4, hipMemcpyDeviceToHost, stream_));   // greedy sample_token reads this copy
    return 0;
}

// ====================================================================================================================
// scoring: log-probabilities of given tokens from the prompt pass (engine.hpp)
// ====================================================================================================================
void Engine::score_alloc() {
    const int need = max_rows_ + MAX_CONVERSATIONS;
    if (score_buf_ && score_cap_ >= need) return;
    HIP_CHECK(hipStreamSynchronize(stream_));
    reset_all(score_buf_, score_tgt_, score_greedy_, score_lp_, score_glp_); score_cap_ = 0;
    DevPtr<float> buf((size_t)SCORE_ROWS * llm_.n_vocab * 4), lp((size_t)need * 4), glp((size_t)need * 4); DevPtr<int> tgt((size_t)need * 4), greedy((size_t)need * 4);   // all five or none
    score_buf_ = std::move(buf); score_tgt_ = std::move(tgt); score_greedy_ = std::move(greedy); score_lp_ = std::move(lp); score_glp_ = std::move(glp);
    score_cap_ = need;
}
Engine::ScoreReq Engine::score_request(const std::vector<int> &targets, int top_n, float *h_logits) {
    ScoreReq rq;
    rq.first = (int)targets.size();
    for (int r = 0; r < (int)targets.size(); r++) if (targets[(size_t)r] >= 0) { rq.first = std::min(rq.first, r); rq.end = r + 1; }
    if (rq.end <= rq.first) return rq;
    HIP_CHECK(hipMemcpyAsync(score_tgt_, targets.data(), targets.size() * 4, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    rq.targets = score_tgt_; rq.logprob = score_lp_; rq.greedy = score_greedy_; rq.greedy_logprob = score_glp_;
    rq.h_logits = h_logits; rq.top_n = top_n;
    return rq;
}
// The scored rows of the pass that is being enqueued: x_ holds every row's residual once the layers are done.  Tiles of SCORE_ROWS rows: final norm + output matrix
// into score_buf_ (parity mode: the oracle-order preparation and mat-mul, as forward_ref's prompt rows), k_logprob_rows, the optional copy of the tile to the host.
void Engine::score_rows(const ScoreReq &rq, hipStream_t s) {
    const int E = (int)llm_.n_embd, V = (int)llm_.n_vocab;
    for (int r0 = rq.first; r0 < rq.end; r0 += SCORE_ROWS) {
        const int rows = std::min(SCORE_ROWS, rq.end - r0);
        const float *xr = x_ + (size_t)r0 * E;
        if (parity_) {
            launch_rms_quant(xr, norm_, rows, E, act_, act_mask_for(output_.type), s, true);
            const QWeight *Wo[1] = {&output_}; float *Yo[1] = {score_buf_};
            if (!(rows >= 5 && launch_mmq2_set(Wo, Yo, nullptr, 1, act_, rows, V, tune_, s, nullptr, 1))) launch_mul_mat_ref(output_, act_, rows, score_buf_, V, nullptr, tune_, s);
        } else {
            const Prep p_rows{1, xr, norm_};
            mul_mat(output_, rows, score_buf_, V, nullptr, s, &p_rows, false, "score");
        }
        launch_logprob_rows(score_buf_, V, V, rows, rq.targets + r0, rq.logprob + r0, rq.greedy + r0, rq.greedy_logprob + r0, s);
        if (rq.top_n && !launch_topn_rows(score_buf_, V, V, rows, nullptr, rq.top_n, rq.targets + r0, topn_ids() + (size_t)r0 * rq.top_n, topn_lp() + (size_t)r0 * rq.top_n,
                                          topn_rank() + r0, topn_tlp() + r0, s))
            throw HipError{hipErrorInvalidValue, "top-N launch refused", __FILE__, __LINE__};
        if (rq.h_logits) HIP_CHECK(hipMemcpyAsync(rq.h_logits + (size_t)(r0 - rq.first) * V, score_buf_, (size_t)rows * V * 4, hipMemcpyDeviceToHost, s));
    }
}
// Entry 0 of a conversation: one launch of the kernel on its logits_ row from before the call (result slot max_rows_ + idx); the no-logits values otherwise.
// The copies land by the caller's next synchronisation.
void Engine::score_entry0(int slot, int idx, int target, float *logprob, int *greedy, float *greedy_logprob, float *logits_out, const TopOut *top) {
    const size_t V = llm_.n_vocab;
    if (!conv_[(size_t)slot].has_logits) {
        *logprob = 0.0f; if (greedy) *greedy = -1; if (greedy_logprob) *greedy_logprob = 0.0f;
        if (logits_out) memset(logits_out, 0, V * 4);
        if (top) { *top->rank = -1; for (int j = 0; j < top->top_n; j++) { top->top_ids[j] = -1; top->top_lp[j] = 0.0f; } }
        return;
    }
    const int at = max_rows_ + idx;
    const float *row = logits_ + (size_t)slot * V;
    launch_set_int(score_tgt_ + at, target, stream_);
    launch_logprob_rows(row, (int)V, (int)V, 1, score_tgt_ + at, score_lp_ + at, score_greedy_ + at, score_glp_ + at, stream_);
    HIP_CHECK(hipMemcpyAsync(logprob, score_lp_ + at, 4, hipMemcpyDeviceToHost, stream_));
    if (greedy) HIP_CHECK(hipMemcpyAsync(greedy, score_greedy_ + at, 4, hipMemcpyDeviceToHost, stream_));
    if (greedy_logprob) HIP_CHECK(hipMemcpyAsync(greedy_logprob, score_glp_ + at, 4, hipMemcpyDeviceToHost, stream_));
    if (logits_out) HIP_CHECK(hipMemcpyAsync(logits_out, row, V * 4, hipMemcpyDeviceToHost, stream_));
    if (top) {
        const size_t o = (size_t)at * top->top_n, nb = (size_t)top->top_n * 4;
        if (!launch_topn_rows(row, (int)V, (int)V, 1, nullptr, top->top_n, score_tgt_ + at, topn_ids() + o, topn_lp() + o, topn_rank() + at, topn_tlp() + at, stream_))
            throw HipError{hipErrorInvalidValue, "top-N launch refused", __FILE__, __LINE__};
        HIP_CHECK(hipMemcpyAsync(top->top_ids, topn_ids() + o, nb, hipMemcpyDeviceToHost, stream_));
        HIP_CHECK(hipMemcpyAsync(top->top_lp, topn_lp() + o, nb, hipMemcpyDeviceToHost, stream_));
        HIP_CHECK(hipMemcpyAsync(top->rank, topn_rank() + at, 4, hipMemcpyDeviceToHost, stream_));
    }
}
// The checks come before anything is evaluated or queued.  The chunks are flush()'s chunks without the prefix store; a chunk whose rows all predict a given token
// (every chunk but the last) scores all its rows, the last chunk all but its last row -- which, when it is the chunk's only row, leaves the captured decode step.
int Engine::score_tokens(const int *tokens, int n, float *logprob, int *greedy, float *greedy_logprob, float *logits_out) {
    return score_tokens_impl("score_tokens", tokens, n, logprob, greedy, greedy_logprob, logits_out, nullptr);
}
int Engine::score_tokens_top(const int *tokens, int n, int top_n, float *logprob, int *rank, int *top_ids, float *top_lp) {
    TopOut top; top.top_n = top_n; top.top_ids = top_ids; top.top_lp = top_lp; top.rank = rank;
    return score_tokens_impl("score_tokens_top", tokens, n, logprob, nullptr, nullptr, nullptr, &top);
}
// top: entry i's alternatives at top_ids / top_lp + i * top_n, its rank at rank + i
int Engine::score_tokens_impl(const char *name, const int *tokens, int n, float *logprob, int *greedy, float *greedy_logprob, float *logits_out, const TopOut *top) {
    auto fail = [name](const std::string &what) { set_last_error(std::string(name) + ": " + what); return 1; };
    if (!tokens || !logprob) return fail("tokens and logprob_out are required");
    if (n < 1) return fail("n < 1");
    const int V = (int)llm_.n_vocab;
    if (top && (!top->rank || !top->top_ids || !top->top_lp)) return fail("rank_out, top_ids_out and top_logprobs_out are required");
    if (top && (top->top_n < 1 || top->top_n > TOPN_MAX || top->top_n > V)) return fail("top_n outside 1 .. min(64, n_vocab)");
    for (int i = 0; i < n; i++) if (tokens[i] < 0 || tokens[i] >= V) return fail("token id out of range");
    if (weights_missing()) return fail(last_error());
    Conversation &cv = conv_[(size_t)cur_];
    if (cv.n_past + n > n_ctx_ && make_room(n)) return fail("context overflow: n_past + n_tokens > n_ctx");
    if (flush()) return fail("the queued rows could not be evaluated: " + last_error());
    score_alloc();
    if (top) topn_alloc();
    const int tn = top ? top->top_n : 0;
    score_entry0(cur_, 0, tokens[0], logprob, greedy, greedy_logprob, logits_out, top);
    std::vector<int> tgt;
    try {
        for (int i = 0; i < n; i += max_chunk_) {
            const int N = std::min(max_chunk_, n - i), nt = std::min(N, n - 1 - i);   // rows i .. i + N - 1; row j predicts tokens[j + 1]
            tgt.assign(tokens + i + 1, tokens + i + 1 + nt); tgt.resize((size_t)N, -1);
            const ScoreReq rq = score_request(tgt, tn, logits_out ? logits_out + (size_t)(i + 1) * V : nullptr);   // rows [0, nt); none when nt == 0
            const int rc = eval_chunk(tokens + i, N, nullptr, rq.end > rq.first ? &rq : nullptr);
            cv.drop_queue();                                                 // (nothing is queued: n_past = n_committed)
            if (rc) return fail("a pass failed: " + last_error());
            if (nt > 0) {
                HIP_CHECK(hipMemcpyAsync(logprob + i + 1, score_lp_, (size_t)nt * 4, hipMemcpyDeviceToHost, stream_));
                if (greedy) HIP_CHECK(hipMemcpyAsync(greedy + i + 1, score_greedy_, (size_t)nt * 4, hipMemcpyDeviceToHost, stream_));
                if (greedy_logprob) HIP_CHECK(hipMemcpyAsync(greedy_logprob + i + 1, score_glp_, (size_t)nt * 4, hipMemcpyDeviceToHost, stream_));
                if (top) {
                    const size_t o = (size_t)(i + 1) * tn, nb = (size_t)nt * tn * 4;
                    HIP_CHECK(hipMemcpyAsync(top->top_ids + o, topn_ids(), nb, hipMemcpyDeviceToHost, stream_));
                    HIP_CHECK(hipMemcpyAsync(top->top_lp + o, topn_lp(), nb, hipMemcpyDeviceToHost, stream_));
                    HIP_CHECK(hipMemcpyAsync(top->rank + i + 1, topn_rank(), (size_t)nt * 4, hipMemcpyDeviceToHost, stream_));
                }
            }
        }
        HIP_CHECK(hipStreamSynchronize(stream_));
    } catch (...) { cv.drop_queue(); throw; }
    return 0;
}
// ====================================================================================================================
// top-N alternatives (engine.hpp)
// ====================================================================================================================
void Engine::topn_alloc() {
    score_alloc();
    if (topn_d_ && topn_cap_ >= score_cap_) return;
    HIP_CHECK(hipStreamSynchronize(stream_));
    reset_all(topn_d_, topn_h_, topn_in_, topn_hin_, topn_ev_); topn_cap_ = 0; topn_m_ = 0;
    const size_t words = (size_t)score_cap_ * (2 * TOPN_MAX + 2);
    DevPtr<int> d(words * 4), in(2 * MAX_CONVERSATIONS * 4); PinPtr<int> h(words * 4), hin(2 * MAX_CONVERSATIONS * 4); OwnedEvent ev(0);   // all five or none
    topn_d_ = std::move(d); topn_h_ = std::move(h); topn_in_ = std::move(in); topn_hin_ = std::move(hin); topn_ev_ = std::move(ev);
    topn_cap_ = score_cap_;
}
// One launch over the logits_ rows of the listed conversations that hold logits (targets: one per listed conversation, -1 = none), the packed results' copy to the
// pinned mirror and the event behind it.  The caller has synchronised the stream since the previous slot call's collect (the pinned inputs are free).
void Engine::topn_slots_launch(const int *slots, int n, int top_n, const int *targets) {
    topn_alloc();
    int m = 0;
    for (int i = 0; i < n; i++) if (conv_[(size_t)slots[i]].has_logits) { topn_hin_[m] = slots[i]; topn_hin_[MAX_CONVERSATIONS + m] = targets ? targets[i] : -1; topn_map_[m] = i; m++; }
    topn_m_ = m;
    if (!m) return;
    const int V = (int)llm_.n_vocab;
    HIP_CHECK(hipMemcpyAsync(topn_in_, topn_hin_, 2 * MAX_CONVERSATIONS * 4, hipMemcpyHostToDevice, stream_));
    int *ids = topn_d_; float *lp = reinterpret_cast<float *>(topn_d_ + (size_t)m * top_n); int *rk = topn_d_ + 2 * (size_t)m * top_n; float *tlp = reinterpret_cast<float *>(rk + m);
    if (!launch_topn_rows(logits_, V, V, m, topn_in_, top_n, topn_in_ + MAX_CONVERSATIONS, ids, lp, rk, tlp, stream_)) throw HipError{hipErrorInvalidValue, "top-N launch refused", __FILE__, __LINE__};
    HIP_CHECK(hipMemcpyAsync(topn_h_, topn_d_, (size_t)m * (2 * top_n + 2) * 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipEventRecord(topn_ev_, stream_));
}
// Waits for that copy and hands the rows out in slot-list order; a conversation that held no logits: ids -1, log-probabilities 0, rank -1.
void Engine::topn_slots_collect(int n, int top_n, int *top_ids, float *top_lp, float *logprob, int *rank) {
    for (int i = 0; i < n; i++) {
        for (int j = 0; j < top_n; j++) { top_ids[(size_t)i * top_n + j] = -1; top_lp[(size_t)i * top_n + j] = 0.0f; }
        if (logprob) logprob[i] = 0.0f;
        if (rank) rank[i] = -1;
    }
    const int m = topn_m_;
    topn_m_ = 0;
    if (!m) return;
    HIP_CHECK(hipEventSynchronize(topn_ev_));
    const int *ids = topn_h_, *rk = topn_h_ + 2 * (size_t)m * top_n;
    const float *lp = reinterpret_cast<const float *>(topn_h_ + (size_t)m * top_n), *tlp = reinterpret_cast<const float *>(rk + m);
    for (int r = 0; r < m; r++) {
        const int i = topn_map_[r];
        memcpy(top_ids + (size_t)i * top_n, ids + (size_t)r * top_n, (size_t)top_n * 4); memcpy(top_lp + (size_t)i * top_n, lp + (size_t)r * top_n, (size_t)top_n * 4);
        if (logprob) logprob[i] = tlp[r];
        if (rank) rank[i] = rk[r];
    }
}
int Engine::top_logprobs(const int *slots, int n, int top_n, const int *targets, int *top_ids, float *top_lp, float *logprob, int *rank) {
    auto fail = [](const std::string &what) { set_last_error("top_logprobs: " + what); return 1; };
    const int V = (int)llm_.n_vocab;
    if (const int bad = check_slots(slots, n)) return fail(bad == 1 ? "bad slot list" : "conversations must be distinct and in range");
    if (!top_ids || !top_lp) return fail("top_ids_out and top_logprobs_out are required");
    if (top_n < 1 || top_n > TOPN_MAX || top_n > V) return fail("top_n outside 1 .. min(64, n_vocab)");
    if (targets) for (int i = 0; i < n; i++) if (targets[i] < -1 || targets[i] >= V) return fail("target id out of range");
    if (weights_missing()) return fail(last_error());
    if (prefill_batch(slots, n)) return fail("the queued rows could not be evaluated: " + last_error());
    HIP_CHECK(hipStreamSynchronize(stream_));
    topn_slots_launch(slots, n, top_n, targets);
    topn_slots_collect(n, top_n, top_ids, top_lp, logprob, rank);
    return 0;
}
int Engine::decode_batch_top(const int *slots, int n, const SampleParams &p, int *ids_out, const TopOut &top) {
    auto fail = [](const std::string &what) { set_last_error("end_chat_batch_top: " + what); return 1; };
    const int V = (int)llm_.n_vocab;
    if (const int bad = check_slots(slots, n)) return fail(bad == 1 ? "bad slot list" : "conversations must be distinct and in range");
    if (!ids_out || !top.top_ids || !top.top_lp || !top.logprob || !top.rank) return fail("ids_out, logprob_out, rank_out, top_ids_out and top_logprobs_out are required");
    if (top.top_n < 1 || top.top_n > TOPN_MAX || top.top_n > V) return fail("top_n outside 1 .. min(64, n_vocab)");
    if (weights_missing()) return fail(last_error());
    if (decode_batch(slots, n, p, ids_out, nullptr, &top)) return fail(last_error());
    return 0;
}
int Engine::score_batch(const int *slots, int n, const int *tokens, const int *counts, float *logprob, int *greedy, float *greedy_logprob) {
    auto fail = [](const std::string &what) { set_last_error("score_batch: " + what); return 1; };
    const int V = (int)llm_.n_vocab;
    if (const int bad = check_slots(slots, n)) return fail(bad == 1 ? "bad slot list" : "conversations must be distinct and in range");
    if (!tokens || !counts || !logprob) return fail("tokens, counts and logprob_out are required");
    size_t total = 0;
    for (int i = 0; i < n; i++) { if (counts[i] < 1) return fail("every count must be >= 1"); total += (size_t)counts[i]; }
    for (size_t i = 0; i < total; i++) if (tokens[i] < 0 || tokens[i] >= V) return fail("token id out of range");
    // make_room's own rule, asked before anything is evaluated: past it, make_room below can only fail with the device (its shift arguments are in range by then)
    for (int i = 0; i < n; i++)
        if (conv_[(size_t)slots[i]].n_past + counts[i] > n_ctx_ && !shift_allows(counts[i])) return fail("context overflow: n_past + n_tokens > n_ctx");
    if (weights_missing()) return fail(last_error());
    const SelectScope restore(this);
    if (parity_ || trace_file_) {   // as prefill_batch: the oracle-order pass is the single-conversation one
        size_t off = 0;
        for (int i = 0; i < n; i++) {
            cur_ = slots[i];
            // (the arguments were checked above: what can still fail is a pass on the device -- the conversations before this one keep what they evaluated, like
            // prefill_batch's per-conversation flush)
            if (score_tokens(tokens + off, counts[i], logprob + off, greedy ? greedy + off : nullptr, greedy_logprob ? greedy_logprob + off : nullptr, nullptr)) return fail(last_error());
            off += (size_t)counts[i];
        }
        return 0;
    }
    if (prefill_batch(slots, n)) return fail("the queued rows could not be evaluated: " + last_error());
    for (int i = 0; i < n; i++) { cur_ = slots[i]; if (conv_[(size_t)cur_].n_past + counts[i] > n_ctx_ && make_room(counts[i])) return fail("context overflow: the automatic shift failed"); }
    score_alloc();
    ScoreOut so; so.logprob = logprob; so.greedy = greedy; so.greedy_logprob = greedy_logprob;
    size_t off = 0;
    for (int i = 0; i < n; i++) {
        so.off[slots[i]] = (int)off;
        score_entry0(slots[i], i, tokens[off], logprob + off, greedy ? greedy + off : nullptr, greedy_logprob ? greedy_logprob + off : nullptr, nullptr);
        off += (size_t)counts[i];
    }
    off = 0;
    for (int i = 0; i < n; i++) {
        Conversation &cv = conv_[(size_t)slots[i]];
        cv.pend_tok.assign(tokens + off, tokens + off + counts[i]); cv.pend_embd.clear();
        cv.n_past += counts[i];
        off += (size_t)counts[i];
    }
    try {
        if (prefill_packed(slots, n, &so)) { drop_queues(slots, n); return fail("a pass failed: " + last_error()); }
        HIP_CHECK(hipStreamSynchronize(stream_));
    } catch (...) { drop_queues(slots, n); throw; }
    return 0;
}

// ====================================================================================================================
// image path
// ====================================================================================================================
// B images in ONE pass over the vision weights (B <= VISION_BATCH_MAX): every GEMM / LayerNorm runs on B x 257 (ViT) or B x 32 (Q-Former) rows,
// attention per image (grid z).  Per output element the arithmetic does not depend on B (one wave accumulates one 32x32 tile over K in a fixed
// order), so image b of a batch equals the same image encoded alone bit for bit
// (tests/test_gpu_parity.py::test_batched_image_encode_is_bit_identical).
int Engine::encode_images(const float *const *chw, int B, float *const *out) {
    if (B < 1 || B > VISION_BATCH_MAX) { set_last_error("encode_images: batch size out of range"); return E_ImageSize; }
    if (weights_missing()) return E_LoadModelFileHeader;
    // MINIGPT4_PARITY: the oracle's accumulation order, image embedding bit-identical to oracle/refcpu.c
    if (parity_) return encode_images_ref(chw, B, out);
    if (v_generic_) return encode_images_generic(chw, B, out);
    hipStream_t s = stream_;
    const int D = v_D_, M = v_M_, NQ = v_nq_, H = 768;
    const int R = B * 257, RQ = B * NQ;                                    // rows of the ViT / Q-Former activations
    hipEvent_t ea, eb; HIP_CHECK(hipEventCreate(&ea)); HIP_CHECK(hipEventCreate(&eb));
    for (int b = 0; b < B; b++) HIP_CHECK(hipMemcpyAsync(vi_img_ + (size_t)b * 3 * 224 * 224, chw[b], 3 * 224 * 224 * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipEventRecord(ea, s));
    // patch embedding: conv 14x14/14 as an f16 GEMM over im2col'd patches (ggml_conv_2d, minigpt4.cpp:1059) + bias
    launch_im2col(vi_img_, vi_patches_, 592, s, B);
    launch_gemm_f16(vi_patches_, 592, v_patch_w_, 592, B * 256, D, 592, v_patch_b_, nullptr, false, tabs_, vi_pe_, nullptr, D, tune_, s);
    launch_assemble_embeddings(v_cls_, vi_pe_, v_pos_, D, vi_x_, s, B);
    const float scale = 1.0f / sqrtf(88.0f);
    // ViT blocks.  attn.proj and mlp.fc2 (N = D: fewer 64x64 tiles than CUs, and fc2 has the longest K) run split-K; their deterministic reduce
    // also adds bias + residual and applies the LayerNorm that follows (norm2, the next block's norm1, ln_vision after the last block).
    const int sp = gemm_split_slices(D, splitk_proj_), sf = gemm_split_slices(M, splitk_fc2_);
    const size_t slab = (size_t)R * D;
    if (!vblocks_.empty()) launch_layernorm(vi_x_, vblocks_[0].n1w, vblocks_[0].n1b, R, D, nullptr, vi_ln_h_, s);
    for (size_t ib = 0; ib < vblocks_.size(); ib++) {
        const VBlock &b = vblocks_[ib];
        const bool last = ib + 1 == vblocks_.size();
        const float *nw = last ? v_lnv_w_ : vblocks_[ib + 1].n1w, *nb = last ? v_lnv_b_ : vblocks_[ib + 1].n1b;
        __half *nout = last ? vi_img_h_ : vi_ln_h_;
        if (qkv_head_major_) {   // q | k | v stored [3][head][R][88]: every head's rows contiguous for the attention kernel (round 6; MINIGPT4_QKV_HEAD_MAJOR=0: rows of 3 x D, A/B, bit-identical)
            launch_gemm_f16_head_major(vi_ln_h_, D, b.qkv_w, D, R, 3 * D, D, b.qkv_b, tabs_, vi_qkv_, D, 88, tune_, s);
            launch_attn_f32(vi_qkv_, 88, vi_qkv_ + (size_t)D * R, vi_qkv_ + (size_t)2 * D * R, 88, 257, 257, v_heads_, 88, scale, 0.0f, tabs_vis_, nullptr, vi_att_h_, D, tune_, s, B, R * 88, R * 88);
        } else {
        launch_gemm_f16(vi_ln_h_, D, b.qkv_w, D, R, 3 * D, D, b.qkv_b, nullptr, false, tabs_, vi_qkv_, nullptr, 3 * D, tune_, s);
        launch_attn_f32(vi_qkv_, 3 * D, vi_qkv_ + D, vi_qkv_ + 2 * D, 3 * D, 257, 257, v_heads_, 88, scale, 0.0f, tabs_vis_, nullptr, vi_att_h_, D, tune_, s, B);
        }
        if (sp > 1) {
            launch_gemm_f16_splitk(vi_att_h_, D, b.proj_w, D, R, D, D, sp, vi_slab_, slab, D, tune_, s);
            launch_splitk_reduce_ln(vi_slab_, sp, slab, b.proj_b, vi_x_, R, D, vi_x_, b.n2w, b.n2b, nullptr, vi_ln_h_, s);
        } else {
            launch_gemm_f16(vi_att_h_, D, b.proj_w, D, R, D, D, b.proj_b, vi_x_, false, tabs_, vi_x_, nullptr, D, tune_, s);
            launch_layernorm(vi_x_, b.n2w, b.n2b, R, D, nullptr, vi_ln_h_, s);
        }
        launch_gemm_f16(vi_ln_h_, D, b.fc1_w, D, R, M, D, b.fc1_b, nullptr, true, tabs_vis_, nullptr, vi_mlp_h_, M, tune_, s);
        if (sf > 1) {
            launch_gemm_f16_splitk(vi_mlp_h_, M, b.fc2_w, M, R, D, M, sf, vi_slab_, slab, D, tune_, s);
            launch_splitk_reduce_ln(vi_slab_, sf, slab, b.fc2_b, vi_x_, R, D, vi_x_, nw, nb, nullptr, nout, s);
        } else {
            launch_gemm_f16(vi_mlp_h_, M, b.fc2_w, M, R, D, M, b.fc2_b, vi_x_, false, tabs_, vi_x_, nullptr, D, tune_, s);
            launch_layernorm(vi_x_, nw, nb, R, D, nullptr, nout, s);
        }
    }
    if (vblocks_.empty()) launch_layernorm(vi_x_, v_lnv_w_, v_lnv_b_, R, D, nullptr, vi_img_h_, s);
    // Q-Former (masks are all-zero).  Its GEMMs have 32 rows per image: the skinny-M kernel (MINIGPT4_QF_SKINNY=0: the
    // 64x64-tile kernel, A/B)
    auto qgemm = [&](const __half *A, int lda, const __half *W, int ldw, int Mr, int N, int K, const float *bias, const float *residual, bool gelu, float *o, __half *oh, int ldo) {
        if (!(qf_skinny_ && launch_gemm_f16_skinny(A, lda, W, ldw, Mr, N, K, bias, residual, gelu, tabs_vis_, o, oh, ldo, s))) launch_gemm_f16(A, lda, W, ldw, Mr, N, K, bias, residual, gelu, tabs_vis_, o, oh, ldo, tune_, s);
    };
    // a 768-wide dense / output layer + residual + the LayerNorm behind it (NNSelfAttention's output block, NNBertEncoderLayer's query FFN output: minigpt4.cpp:1365-1400,
    // 1430-1461).  Round 6: K split over 2 (K = 768) or 4 (K = 3072) workgroups per tile with the LayerNorm in the slab reduce (qf_dense_ln below).
    auto dense_ln = [&](const __half *A, int lda, const __half *W, int K, const float *bias, const float *residual, const float *lw, const float *lb, float *o, __half *oh) {
        qf_dense_ln(A, lda, W, K, bias, residual, lw, lb, o, oh, RQ, s);
    };
    // the cross-attention K | V projections of every cross layer depend on the image features only (minigpt4.cpp:1148-1155): ONE [R x D] . [D x
    // n_cross * 1536] launch here instead of one per cross layer inside the loop; layer i reads its [R][1536] column slice (row stride n_cross *
    // 1536)
    const bool hoist = kv_hoist_ && v_ncross_ > 0 && v_kv_all_w_;
    const int ldkv = hoist ? v_ncross_ * 2 * H : 2 * H;
    if (hoist) launch_gemm_f16(vi_img_h_, D, v_kv_all_w_, D, R, v_ncross_ * 2 * H, D, v_kv_all_b_, nullptr, false, tabs_, vi_kv_, nullptr, ldkv, tune_, s);
    const bool folded = qf_fold_ && qf_folded_;                            // layer 0's image-independent head was evaluated at load time (fold_qformer_constants)
    if (!folded) launch_layernorm(vi_qtok_rep_, v_qeln_w_, v_qeln_b_, RQ, H, vi_hs_, vi_hs_h_, s);
    for (size_t il = 0; il < qlayers_.size(); il++) {
        const QLayer &L = qlayers_[il];
        const bool pre = folded && il == 0;
        const float *a1 = pre ? vi_c_a1_ : vi_a1_; const __half *a1_h = pre ? vi_c_a1_h_ : vi_a1_h_;
        if (!pre) {
            qgemm(vi_hs_h_, H, L.self.q_w, H, RQ, 3 * H, H, L.self.q_b, nullptr, false, vi_qq_, nullptr, 3 * H);
            launch_attn_f32(vi_qq_, 3 * H, vi_qq_ + H, vi_qq_ + 2 * H, 3 * H, NQ, NQ, 12, 64, 0.0f, 8.0f, tabs_vis_, nullptr, vi_ctx_h_, H, tune_, s, B);
            dense_ln(vi_ctx_h_, H, L.self.dense_w, H, L.self.dense_b, vi_hs_, L.self.ln_w, L.self.ln_b, vi_a1_, vi_a1_h_);
        }
        const float *ao = a1; const __half *ao_h = a1_h;
        if (L.has_cross) {
            const float *cq = pre ? vi_c_qq_ : vi_qq_;
            if (!pre) qgemm(vi_a1_h_, H, L.cross.q_w, H, RQ, H, H, L.cross.q_b, nullptr, false, vi_qq_, nullptr, H);
            const float *kv = hoist ? vi_kv_ + (size_t)L.cross_idx * 2 * H : vi_kv_;
            if (!hoist) launch_gemm_f16(vi_img_h_, D, L.cross.kv_w, D, R, 2 * H, D, L.cross.kv_b, nullptr, false, tabs_, vi_kv_, nullptr, 2 * H, tune_, s);
            launch_attn_f32(cq, H, kv, kv + H, ldkv, NQ, 257, 12, 64, 0.0f, 8.0f, tabs_vis_, nullptr, vi_ctx_h_, H, tune_, s, B);
            dense_ln(vi_ctx_h_, H, L.cross.dense_w, H, L.cross.dense_b, a1, L.cross.ln_w, L.cross.ln_b, vi_a2_, vi_a2_h_);
            ao = vi_a2_; ao_h = vi_a2_h_;
        }
        qgemm(ao_h, H, L.inter_w, H, RQ, v_qi_, H, L.inter_b, nullptr, true, nullptr, vi_im_h_, v_qi_);
        dense_ln(vi_im_h_, v_qi_, L.out_w, v_qi_, L.out_b, ao, L.oln_w, L.oln_b, vi_hs_, vi_hs_h_);
    }
    qgemm(vi_hs_h_, H, v_proj_w_, H, RQ, v_out_, H, v_proj_b_, nullptr, false, vi_out_, nullptr, v_out_);
    HIP_CHECK(hipEventRecord(eb, s));
    for (int b = 0; b < B; b++) HIP_CHECK(hipMemcpyAsync(out[b], vi_out_ + (size_t)b * NQ * v_out_, (size_t)NQ * v_out_ * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipEventElapsedTime(&last_encode_ms_, ea, eb));
    HIP_IGNORE(hipEventDestroy(ea)); HIP_IGNORE(hipEventDestroy(eb));
    return E_None;
}
int Engine::encode_image(const float *chw, float *out) { return encode_images(&chw, 1, &out); }

// out (fp32) / out_h (fp16) = LayerNorm(residual + (bias + A . W^T)) for a 768-wide layer of the Q-Former, `rows` rows.  The whole-K skinny launch is 48 workgroups on 256
// CUs, each pulling 32 rows of A and 16 of W over the full K through one CU's load path, followed by a standalone LayerNorm launch; here the K range is split over 2 (K = 768)
// or 4 (K >= 2048) workgroups per tile (raw partial sums into slabs) and the deterministic slab reduce adds bias + residual and normalises -- the same two launches, the
// first one 2-4 x wider.  The slice count depends on K only, never on the rows: image b of a batch equals the image encoded alone.  MINIGPT4_QF_SPLITK=0: the round 2-5 form.
void Engine::qf_dense_ln(const __half *A, int lda, const __half *W, int K, const float *bias, const float *residual, const float *ln_w, const float *ln_b, float *out, __half *out_h,
                         int rows, hipStream_t s) {
    const int H = 768, slices = K >= 2048 ? 4 : 2;
    if (qf_splitk_ && qf_skinny_ && launch_gemm_f16_skinny_splitk(A, lda, W, K, rows, H, K, slices, vi_slab_, (size_t)rows * H, H, s)) {
        launch_splitk_reduce_ln(vi_slab_, slices, (size_t)rows * H, bias, residual, rows, H, nullptr, ln_w, ln_b, out, out_h, s);
        return;
    }
    if (!(qf_skinny_ && launch_gemm_f16_skinny(A, lda, W, K, rows, H, K, bias, residual, false, tabs_, vi_d_, nullptr, H, s))) launch_gemm_f16(A, lda, W, K, rows, H, K, bias, residual, false, tabs_, vi_d_, nullptr, H, tune_, s);
    launch_layernorm(vi_d_, ln_w, ln_b, rows, H, out, out_h, s);
}

// What the Q-Former computes before it first looks at the image: hs = LayerNorm(query tokens) (minigpt4.cpp:2236-2246), layer 0's self-attention
// block on hs (NNSelfAttention + residual + LayerNorm, minigpt4.cpp:1365-1400) and, when layer 0 has cross-attention, its query projection.  None of
// it depends on the image, so it is evaluated ONCE here -- by the very launches encode_images would issue for one image (32 rows) -- and replicated
// for the images of a batch: six launches less per encode, bit-identical embeddings.  Fast f16 path only (parity mode and quantised / f32 vision
// files run their own chains).
void Engine::fold_qformer_constants() {
    qf_folded_ = false;
    if (!qf_fold_ || v_generic_ || qlayers_.empty() || !vi_c_a1_) return;
    hipStream_t s = stream_;
    const int H = 768, NQ = v_nq_;
    const QLayer &L = qlayers_[0];
    auto qgemm = [&](const __half *A, int lda, const __half *W, int ldw, int Mr, int N, int K, const float *bias, const float *residual, bool gelu, float *o, __half *oh, int ldo) {
        if (!(qf_skinny_ && launch_gemm_f16_skinny(A, lda, W, ldw, Mr, N, K, bias, residual, gelu, tabs_vis_, o, oh, ldo, s))) launch_gemm_f16(A, lda, W, ldw, Mr, N, K, bias, residual, gelu, tabs_vis_, o, oh, ldo, tune_, s);
    };
    launch_layernorm(vi_qtok_rep_, v_qeln_w_, v_qeln_b_, NQ, H, vi_hs_, vi_hs_h_, s);
    qgemm(vi_hs_h_, H, L.self.q_w, H, NQ, 3 * H, H, L.self.q_b, nullptr, false, vi_qq_, nullptr, 3 * H);
    launch_attn_f32(vi_qq_, 3 * H, vi_qq_ + H, vi_qq_ + 2 * H, 3 * H, NQ, NQ, 12, 64, 0.0f, 8.0f, tabs_vis_, nullptr, vi_ctx_h_, H, tune_, s, 1);
    qf_dense_ln(vi_ctx_h_, H, L.self.dense_w, H, L.self.dense_b, vi_hs_, L.self.ln_w, L.self.ln_b, vi_c_a1_, vi_c_a1_h_, NQ, s);   // the launches encode_images issues
    if (L.has_cross) qgemm(vi_c_a1_h_, H, L.cross.q_w, H, NQ, H, H, L.cross.q_b, nullptr, false, vi_c_qq_, nullptr, H);
    HIP_CHECK(hipStreamSynchronize(s));
    const size_t n = (size_t)NQ * H;
    for (size_t b = 1; b < (size_t)VISION_BATCH_MAX; b++) {
        HIP_CHECK(hipMemcpy(vi_c_a1_ + b * n, vi_c_a1_, n * 4, hipMemcpyDeviceToDevice)); HIP_CHECK(hipMemcpy(vi_c_a1_h_ + b * n, vi_c_a1_h_, n * 2, hipMemcpyDeviceToDevice));
        if (L.has_cross) HIP_CHECK(hipMemcpy(vi_c_qq_ + b * n, vi_c_qq_, n * 4, hipMemcpyDeviceToDevice));
    }
    qf_folded_ = true;
}

}  // namespace mg4
