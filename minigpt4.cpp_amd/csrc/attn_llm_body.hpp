// NOT a header: the statements of the decode attention body, included INSIDE the two kernels k_attn_llm<HD, FUSED, BATCHED, VS> and k_attn_llm_draft<HD, VS> of
// llm_kernels.hip (description, forms, the list of DRAFT's lines and of VS's: there, above the kernels).  In scope at the point of inclusion: the kernels' parameters (q,
// kin, vin, kc, vc, E, n_past, n_ctx, cos_tab, sin_tab, tb, out, row_slot, seq_stride) and the constants HD, FUSED, BATCHED, DRAFT, VS.
// Why text and not a function template: with the body behind a __device__ function (forceinline or not; __restrict__ or plain parameters; Tables by value, by reference
// or only its exp pointer; indices and position read in the kernel and passed in) hipcc allocates the six fused k_attn_llm one VGPR and 1 ... 9 instructions differently
// from the ISA that was validated and measured -- the optimised IR then differs in one eliminated smin and in inbounds flags of the last reduction; why, not known.
// Included, all twelve instantiations are instruction for instruction what they were (tools/isa_diff.py) -- and stayed so as the VS = 1 forms when VS was added
// (every VS line below is a compile-time `VS == 1 ? the former expression : ...`; tools/isa_diff.py --rename maps the old symbols onto <..., VS = 1>).
// A COPY of this file's DRAFT lines lives in llm_kernels.hip: k_attn_llm_mdraft<HD, VS>, the verify form for several conversations, with (t - r, r) where DRAFT has
// (0, t).  It is a copy so that the instantiations of THIS text stay the validated ISA; its contract is bit-identity with the DRAFT form (tests/test_gpu_draft_batch.py),
// so a change to a DRAFT line here -- operand order, rounding call, loop structure -- has to be made there too.
    static_assert((FUSED || !BATCHED) && (BATCHED || !DRAFT), "BATCHED implies FUSED, DRAFT implies BATCHED");
    static_assert(VS == 1 || (FUSED && (VS == 2 || VS == 4) && (HD / 8) % VS == 0), "the value-column split: fused forms, 2 or 4 workgroups per (head, row)");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int CH = HD / 8, P = AT_THREADS / CH, RM = DRAFT ? DRAFT_ROWS : 1;
    static_assert(!DRAFT || (RM <= P && RM * (HD / 2) <= AT_THREADS), "one prologue thread per (row, rotated pair); at most one LDS key per partition");
    const int h = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    // VS > 1: workgroup blockIdx.z of the VS that share this (head, row) -- all of them do everything up to ph[], then each its own HD / VS output dims.  Its P.V threads are
    // the first AT_THREADS / VS (whole waves): chunk cv of the workgroup's CH / VS, partition pv of the same P.  VS == 1: (cv, pv) = (c, p), every thread.
    constexpr int CHV = (HD / 8) / VS;
    const bool vact = VS == 1 || tid < AT_THREADS / VS;
    int pos_, p0_ = 0;
    if (BATCHED) {
        const int slot = row_slot[DRAFT ? 0 : t];
        p0_ = n_past[slot]; pos_ = DRAFT ? p0_ + t : p0_;
        if (DRAFT && pos_ >= n_ctx) return;
        kc += (size_t)slot * seq_stride; vc += (size_t)slot * seq_stride;
    } else pos_ = *n_past + t;
    MG4_ATTN_PIN();                                               // every argument's load is issued by here, in the position's round trip (llm_kernels.hip, above the kernels)
    const int pos = pos_, p0 = p0_, T = pos + 1;                  // p0: DRAFT only
    const int Tg = FUSED ? pos : T;                               // keys that are not this row's own
    const int Tpad = (T + 7) & ~7;
    float *sc = reinterpret_cast<float *>(smem);                  // [Tpad]                 (the carve-up attn_lds_bytes sizes)
    __half *ph = reinterpret_cast<__half *>(sc + Tpad);           // [Tpad]
    __half *qh = ph + Tpad;                                       // [HD]
    __half *knew = qh + HD, *vnew = knew + RM * HD;               // [RM][HD] each: this row's (DRAFT: rows 0 .. t of the pass)
    float *part = reinterpret_cast<float *>(vnew + RM * HD);      // [P][HD]
    __shared__ float s_red[AT_THREADS / 64];
    __shared__ double s_dred[AT_THREADS / 64];
    const float scale = 1.0f / sqrtf((float)HD);
    const size_t qo = (size_t)t * E + (size_t)h * HD;
    if (FUSED) {
        if (DRAFT) {                                              // one thread per (row r <= t of the pass, rotated pair): rows before t only fill knew / vnew [r]
            if (tid < (t + 1) * (HD / 2)) {
                const int r = tid / (HD / 2), i = tid % (HD / 2), pr = p0 + r;
                const size_t ro = (size_t)r * E + (size_t)h * HD;
                const float c = cos_tab[(size_t)pr * (HD / 2) + i], s = sin_tab[(size_t)pr * (HD / 2) + i];
                const __half2 kr = rope_rot_h2(kin[ro + 2 * i], kin[ro + 2 * i + 1], c, s);
                const __half2 vr = __floats2half2_rn(vin[ro + 2 * i], vin[ro + 2 * i + 1]);
                st_h2(knew + r * HD + 2 * i, kr); st_h2(vnew + r * HD + 2 * i, vr);
                if (r == t) {
                    st_h2(qh + 2 * i, rope_rot_h2(q[qo + 2 * i], q[qo + 2 * i + 1], c, s));
                    const size_t co = (size_t)pos * E + (size_t)h * HD + 2 * i;
                    if (VS == 1 || blockIdx.z == 0) { st_h2(kc + co, kr); st_h2(vc + co, vr); }
                }
            }
        } else if (tid < HD / 2) {                                // one thread per rotated pair of the row
            const int i = tid;
            const float c = cos_tab[(size_t)pos * (HD / 2) + i], s = sin_tab[(size_t)pos * (HD / 2) + i];
            const __half2 qr = rope_rot_h2(q[qo + 2 * i], q[qo + 2 * i + 1], c, s), kr = rope_rot_h2(kin[qo + 2 * i], kin[qo + 2 * i + 1], c, s);
            const __half2 vr = __floats2half2_rn(vin[qo + 2 * i], vin[qo + 2 * i + 1]);
            st_h2(qh + 2 * i, qr); st_h2(knew + 2 * i, kr); st_h2(vnew + 2 * i, vr);
            const size_t co = (size_t)pos * E + (size_t)h * HD + 2 * i;
            if (VS == 1 || blockIdx.z == 0) { st_h2(kc + co, kr); st_h2(vc + co, vr); }   // the append: one workgroup of the VS (the others read rows below pos only)
        }
    } else {
        for (int i = tid; i < HD; i += AT_THREADS) qh[i] = f2h_rn(q[qo + i]);
    }
    __syncthreads();
    unsigned qreg[HD / 2];
#pragma unroll
    for (int i = 0; i < HD / 8; i++) { const int4 v4 = *reinterpret_cast<const int4 *>(qh + 8 * i); qreg[4 * i] = (unsigned)v4.x; qreg[4 * i + 1] = (unsigned)v4.y; qreg[4 * i + 2] = (unsigned)v4.z; qreg[4 * i + 3] = (unsigned)v4.w; }
    auto dot_row = [&](const __half *kr) {
        int4 kk[HD / 8];
#pragma unroll
        for (int i = 0; i < HD / 8; i++) kk[i] = ld16(kr + 8 * i);
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < HD / 8; i++) {
            const unsigned w[4] = {(unsigned)kk[i].x, (unsigned)kk[i].y, (unsigned)kk[i].z, (unsigned)kk[i].w};
#pragma unroll
            for (int e = 0; e < 4; e++) { s = fmaf(h2f_bits(w[e] & 0xFFFF), h2f_bits(qreg[4 * i + e] & 0xFFFF), s); s = fmaf(h2f_bits(w[e] >> 16), h2f_bits(qreg[4 * i + e] >> 16), s); }
        }
        return s * scale;
    };
    // (Measured and not adopted, profiles/r02m_bench_n1.json vs r02k: requesting these K / V rows at kernel entry, before the RoPE prologue and its barrier, with the exp
    // table's live part in LDS and the KV append moved behind the last barrier -- 11.7 us per launch at a context of 430 against 10.9 us for this form; beside LDS-DMA
    // hipcc waits vmcnt(0) for every ordinary load, so the prologue sat out the whole prefetch.)
    // Scores of the cached keys: 16 consecutive lanes share one key row (lane c holds its dims 8 c .. 8 c + 7 -- one 256-byte row per 16 lanes, four whole rows per
    // wave instruction; the round-1 form, a whole row per lane, asked the address path for 64 different cache lines per instruction and grew by ~0.025 us per key), the
    // 8-dim partial dots are added across the 16 lanes with DPP.  Key and value rows of the same (lane, round) sit at the same offset of the two caches, and neither
    // depends on this step's scores: both are requested here, NPRE rounds deep, so they arrive during the dot products / the softmax.
    const int c = tid % CH, p = tid / CH;
    const int cv = VS == 1 ? c : (int)blockIdx.z * CHV + tid % CHV, pv = VS == 1 ? p : tid / CHV;
    const __half *kb = kc + (size_t)h * HD + 8 * c, *vb = vc + (size_t)h * HD + 8 * cv;
    constexpr int NPRE = 16;                        // x P = 32 key partitions: contexts up to 512 need no second round trip
    // loads are clamped to the last row the cache is read at: never a branch, never outside the cache.  DRAFT: rows from p0 on are written by this launch
    const int gmax = DRAFT ? max(p0 - 1, 0) : 0;                  // DRAFT: the last row the cache is read at
    int4 kpre[NPRE], vpre[NPRE];
#pragma unroll
    for (int i = 0; i < NPRE; i++) kpre[i] = ld16(kb + (size_t)min(p + i * P, DRAFT ? gmax : max(Tg - 1, 0)) * E);
    if (vact) {
#pragma unroll
        for (int i = 0; i < NPRE; i++) vpre[i] = ld16(vb + (size_t)min(pv + i * P, DRAFT ? gmax : max(Tg - 1, 0)) * E);
    }
    // DRAFT: this partition's key among the pass's earlier rows, if any: row rl at position jl (jl mod P == p)
    int jl = -1, jlv = -1;                                        // jlv: the same for the P.V roles (VS == 1: jl)
    int4 kl = make_int4(0, 0, 0, 0), vl = kl;
    if (DRAFT) {
        const int rl = (p - p0) & (P - 1), rlv = (pv - p0) & (P - 1);
        jl = rl < t ? p0 + rl : -1; jlv = rlv < t ? p0 + rlv : -1;
        kl = *reinterpret_cast<const int4 *>(knew + min(rl, RM - 1) * HD + 8 * c); vl = *reinterpret_cast<const int4 *>(vnew + min(rlv, RM - 1) * HD + 8 * cv);
    }
    float qd[8];
    unpack8(*reinterpret_cast<const int4 *>(qh + 8 * c), qd);
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NPRE; i++) { const int j = p + i * P; const float s = dot16<CH>(DRAFT && j == jl ? kl : kpre[i], qd, scale); if (j < Tg) { if (c == 0) sc[j] = s; mx = fmaxf(mx, s); } }
    for (int j0 = p + NPRE * P; j0 < Tg; j0 += 8 * P) {      // beyond the prefetch: 8 rows per round trip
        int4 kk[8];
#pragma unroll
        for (int i = 0; i < 8; i++) kk[i] = ld16(kb + (size_t)min(j0 + i * P, DRAFT ? gmax : Tg - 1) * E);
#pragma unroll
        for (int i = 0; i < 8; i++) { const int j = j0 + i * P; const float s = dot16<CH>(DRAFT && j == jl ? kl : kk[i], qd, scale); if (j < Tg) { if (c == 0) sc[j] = s; mx = fmaxf(mx, s); } }
    }
    if (FUSED && tid == AT_THREADS - 1) { const float s = dot_row(knew + (DRAFT ? t : 0) * HD); sc[pos] = s; mx = fmaxf(mx, s); }
    mx = wave_max(mx);
    if ((tid & 63) == 0) s_red[tid >> 6] = mx;
    __syncthreads();
    mx = s_red[0];
#pragma unroll
    for (int i = 1; i < AT_THREADS / 64; i++) mx = fmaxf(mx, s_red[i]);
    double sum = 0.0;
    for (int j = tid; j < T; j += AT_THREADS) { const float v = exp_h(tb.exp, sc[j] - mx); sc[j] = v; sum += (double)v; }
    sum = wave_sum_d(sum);
    if ((tid & 63) == 0) s_dred[tid >> 6] = sum;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < AT_THREADS / 64; i++) tot += s_dred[i];
    const float inv = (float)(1.0 / tot);
    for (int j = tid; j < T; j += AT_THREADS) ph[j] = f2h_rn(sc[j] * inv);
    __syncthreads();
    float o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // pv_acc goes through this lambda, as the kernels always had one here: with the helper called directly from the loops hipcc schedules all twelve k_attn_llm /
    // k_attn_llm_draft instantiations differently (3 ... 5 instructions more, same registers; cause not known) -- they would no longer be the validated ISA.
    auto pv_key = [&](const int4 &vv, const int j) { pv_acc(o, vv, __half2float(ph[j])); };
    if (vact) {                                                   // VS > 1: the other waves skip (wave-uniform; no barrier inside)
#pragma unroll
        for (int i = 0; i < NPRE; i++) { const int j = pv + i * P; if (j < Tg) pv_key(DRAFT && j == jlv ? vl : vpre[i], j); }
        for (int j0 = pv + NPRE * P; j0 < Tg; j0 += 8 * P) {
            int4 vv[8];
#pragma unroll
            for (int i = 0; i < 8; i++) vv[i] = ld16(vb + (size_t)min(j0 + i * P, DRAFT ? gmax : Tg - 1) * E);
#pragma unroll
            for (int i = 0; i < 8; i++) { const int j = j0 + i * P; if (j < Tg) pv_key(DRAFT && j == jlv ? vl : vv[i], j); }
        }
        if (FUSED && pv == P - 1) {
            const float pj = __half2float(ph[pos]);
#pragma unroll
            for (int e = 0; e < 8; e++) o[e] = fmaf(__half2float(vnew[(DRAFT ? t : 0) * HD + 8 * cv + e]), pj, o[e]);
        }
#pragma unroll
        for (int e = 0; e < 8; e++) part[pv * HD + 8 * cv + e] = o[e];
    }
    __syncthreads();
    // the partitions in order 0 .. P - 1, as ever; VS > 1: this workgroup's HD / VS dims
    for (int i = (VS == 1 ? 0 : (int)blockIdx.z * (HD / VS)) + tid; i < (VS == 1 ? HD : ((int)blockIdx.z + 1) * (HD / VS)); i += AT_THREADS) { float s = 0.0f;
#pragma unroll 8
        for (int pp = 0; pp < P; pp++) s += part[pp * HD + i];
        out[qo + i] = s; }
