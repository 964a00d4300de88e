// The bodies the lock-step kernels of stream.hip share with their per-stream forms (k_stream_*_each), as text: each
// is included inside both kernels, once with the lock-step call's scalars in scope and once with the stream's row.
// Text, not a function, because a function would change the lock-step kernels: passing the by-value kernel argument
// struct on makes the compiler load all of it at entry instead of each field where it is used (DESIGN.md K17,
// "Independent streams"), and those kernels are to stay instruction for instruction what they were.
//
// STREAM_BODY_SPEC   one analysis block.  In scope: SpecStreamArgs a; int b (stream); unsigned blk (chunk of SCHUNK
//                    frames, or a.nblk: the stream's new tail)
// STREAM_BODY_COPY   part `part` of ROUTE_X of one video slice's copy.  In scope: RouteArgs a; src; dst; int part, tid
// STREAM_BODY_CLAMP  the causal clamp of a stream's completed slices (one block).  In scope: RouteArgs a; int b, tid;
//                    macros STREAM_K_OLD, STREAM_K_NEW (first slice, count) and STREAM_CLIP(kk) (slice kk's clip in the
//                    network's input)
#if defined(STREAM_BODY_SPEC)
    __shared__ float2 zbuf[SWAVES * FPG * ZS];
    __shared__ float2 twl[640];
    __shared__ v2f ut2[161];       // U = -i W640^k / 2 (untangling)
    __shared__ float2 winl[320];
    __shared__ float4 melw4[NMEL * MW / 4];
    __shared__ int mel_st[NMEL];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int)blk == a.nblk) {   // the new tail: the last TAIL samples received (zeros before sample 0)
        for (int j = tid; j < TAIL; j += 64 * SWAVES) {
            const long long i = a.n_new - TAIL + j;
            a.tail_out[b * (long long)TAIL + j] = i < 0 ? 0.f : stream_sample(a, b, i);
        }
        return;
    }
    for (int i = tid; i < 640; i += 64 * SWAVES) twl[i] = a.twiddle[i];
    for (int k = tid; k < 161; k += 64 * SWAVES) {
        const float2 w = a.twiddle[k];
        ut2[k] = v2f{0.5f * w.y, -0.5f * w.x};
    }
    for (int i = tid; i < 320; i += 64 * SWAVES) winl[i] = reinterpret_cast<const float2*>(a.window)[i];
    for (int i = tid; i < NMEL * MW / 4; i += 64 * SWAVES) melw4[i] = reinterpret_cast<const float4*>(a.mel_weight)[i];
    for (int i = tid; i < NMEL; i += 64 * SWAVES) mel_st[i] = a.mel_start[i];

    const int g = FPG * wave;                                  // this wave's first frame in the block
    const int nf = min(SCHUNK, a.nt - SCHUNK * (int)blk);
    const int ng = max(0, min(FPG, nf - g));
    const long long tw0 = a.t0 + SCHUNK * (long long)blk + g;   // the wave's first frame
    const int f1 = lane >> 4, n1 = lane & 15;
    float2 x[20];
#pragma unroll
    for (int n2 = 0; n2 < 20; ++n2) x[n2] = make_float2(0.f, 0.f);
    if (f1 < ng) {
        const long long s0 = (tw0 + f1) * 160 - 320;
        if (s0 >= a.n_old && s0 + 640 <= a.n_new && (a.Lf < 0 || s0 + 640 <= a.Lf)) {   // all in this call's samples
            const float* p = a.news + b * a.news_stride + (s0 - a.n_old) + 2 * n1;
#pragma unroll
            for (int n2 = 0; n2 < 20; ++n2) x[n2] = make_float2(p[32 * n2], p[32 * n2 + 1]);
        } else {
#pragma unroll
            for (int n2 = 0; n2 < 20; ++n2) {
                const long long i = s0 + 2 * (n1 + 16 * n2);
                x[n2] = make_float2(frame_sample(a, b, i), frame_sample(a, b, i + 1));
            }
        }
    }
    __syncthreads();
    float2* zw = zbuf + wave * FPG * ZS;
    // ---- steps 1 and 2: the 16 x 20 split of k_spec640, wave-local (each wave owns its three frames) ----
    v2f v[20];
    window_frame(v, x, winl, n1);
    if (f1 < ng) dft20_store(v, twl, zw + f1 * ZS, n1);
    wave_lds_sync();
    {
        const int f = lane / 20, k2 = lane - 20 * (lane / 20);
        const bool act = f < ng;
        v2f w[16];
        v2f* zf = reinterpret_cast<v2f*>(zw + min(f, FPG - 1) * ZS);
        if (act) dft16_load(w, zf, k2);
        wave_lds_sync();
        if (act) dft16_store(w, zf, k2);
    }
    wave_lds_sync();
    // ---- step 3: untangling -> the complex frame into the phase ring, its magnitudes into LDS; item = (f, k) ----
    {
        constexpr int IT3 = (FPG * 161 + 63) / 64;   // 8
        float mk[IT3], mm[IT3];
#pragma unroll
        for (int j = 0; j < IT3; ++j) {
            const int it = lane + 64 * j;
            if (it >= ng * 161) break;
            const int f = it / 161, k = it - 161 * f;
            v2f X, Y;
            pk_untangle(reinterpret_cast<const v2f*>(zw + f * ZS), k, ut2, X, Y);
            mk[j] = pk_abs(X);
            mm[j] = pk_abs(Y);
            float2* o = a.phase_ring + ((long long)b * a.R + (int)((tw0 + f) % a.R)) * 321;
            o[k] = make_float2(X.x, X.y);
            if (k != 160) o[320 - k] = make_float2(Y.x, -Y.y);   // X[320 - k] = conj(Y)
        }
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < IT3; ++j) {
            const int it = lane + 64 * j;
            if (it >= ng * 161) break;
            const int f = it / 161, k = it - 161 * f;
            float* mf = reinterpret_cast<float*>(zw + f * ZS);
            mf[k] = mk[j];
            mf[320 - k] = mm[j];
        }
        for (int it = lane; it < FPG * MW; it += 64) {   // bins [321, 321 + MW) are read by the padded band dots
            const int f = it / MW, j = it - MW * f;
            reinterpret_cast<float*>(zw + f * ZS)[321 + j] = 0.f;
        }
        wave_lds_sync();
    }
    // ---- step 4: Slaney mel + dB, item = (m, f) as k_spec640; unclamped, into the frame's slice slot ----
    float fm0 = -INFINITY, fm1 = -INFINITY, fm2 = -INFINITY;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int it = lane + 64 * jj;
        if (it >= FPG * NMEL) break;
        const int m = __umul24(it, 43691) >> 17, f = it - 3 * m;   // m = it / 3 (it < 240)
        if (f >= ng) continue;
        const float* mf = reinterpret_cast<const float*>(zw + f * ZS) + mel_st[m];
        const float acc = band_dot_nq(melw4 + m * (MW / 4), reinterpret_cast<const v2f*>(mf), a.nq[jj]);
        const float db = mel_to_db(acc, a.amin, a.db_floor);
        const long long t = tw0 + f, sl = t / a.spf;
        a.mel_ring[(((long long)b * a.RS + (int)(sl % a.RS)) * NMEL + m) * a.spf + (int)(t - sl * a.spf)] = db;
        fm0 = f == 0 ? fmaxf(fm0, db) : fm0;
        fm1 = f == 1 ? fmaxf(fm1, db) : fm1;
        fm2 = f == 2 ? fmaxf(fm2, db) : fm2;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        fm0 = fmaxf(fm0, __shfl_xor(fm0, o));
        fm1 = fmaxf(fm1, __shfl_xor(fm1, o));
        fm2 = fmaxf(fm2, __shfl_xor(fm2, o));
    }
    if (lane < ng) a.fmax_ring[(long long)b * a.R + (int)((tw0 + lane) % a.R)] = lane == 0 ? fm0 : lane == 1 ? fm1 : fm2;
#elif defined(STREAM_BODY_COPY)
    if (a.vec16) {
        const long long n = a.vbytes / 16;
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        for (long long i = part * 256LL + tid; i < n; i += ROUTE_X * 256LL) d4[i] = s4[i];
    } else {
        const long long n = a.vbytes / 4;
        const unsigned* s1 = reinterpret_cast<const unsigned*>(src);
        unsigned* d1 = reinterpret_cast<unsigned*>(dst);
        for (long long i = part * 256LL + tid; i < n; i += ROUTE_X * 256LL) d1[i] = s1[i];
    }
#elif defined(STREAM_BODY_CLAMP)
    // the floor of slice k is (the maximum over every frame up to its last) - top_db.  Wave w takes the maxima of slices
    // w, w + 4, ..: a lane per frame, then the wave's maximum (a maximum has no order)
    for (int kk = tid >> 6; kk < STREAM_K_NEW; kk += 4) {
        const long long t0 = (STREAM_K_OLD + kk) * a.spf;
        float m = -INFINITY;
        for (int tt = tid & 63; tt < a.spf; tt += 64) m = fmaxf(m, a.fmax_ring[(long long)b * a.R + (int)((t0 + tt) % a.R)]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if ((tid & 63) == 0) slice_max[kk] = m;
    }
    float cur = a.run_max[b];
    __syncthreads();   // the slices' maxima are there, and every thread has read the old running maximum
    const int per = NMEL * a.spf;
    for (int kk = 0; kk < STREAM_K_NEW; ++kk) {   // the prefix maximum, in slice order
        cur = fmaxf(cur, slice_max[kk]);
        const float floor_db = a.top_db >= 0.f ? cur - a.top_db : -INFINITY;
        const float* src = a.mel_ring + ((long long)b * a.RS + (int)((STREAM_K_OLD + kk) % a.RS)) * per;
        const long long d0 = STREAM_CLIP(kk) * per;
        for (int i = tid; i < per; i += 256) {
            const float v = fmaxf(src[i], floor_db);
            a.net_in[d0 + i] = v;
            if (a.mel_out) a.mel_out[d0 + i] = v;
        }
    }
    if (tid == 0) a.run_max[b] = cur;
#else
#error "stream_body.inc: define which body to include"
#endif
