// Experiments (compiled only with -DCNRMA_EXPERIMENTS into libcnrma_hip_exp.so; scripts/ and the bit-identity tests use them;
// the product library carries none of this).  Included by sparse.hip inside its anonymous namespace.

// ================================================================================================================
// Warp-specialised form of the f16x3 stage kernel (round 4).  The ablation of the kernel above (diagnostic ABL build:
// profiles/r04_conv_ablation_S.log) shows its phases ADD UP instead of overlapping -- on the 277 k-row 64 -> 64 layer: loop
// skeleton (barriers + index bookkeeping) 92 us, global loads 110, LDS stores 30-60, fragment reads + MFMAs 100 of 356 --
// because every wave of a block walks through all of them between two block-wide barriers.  Here a block is 8 waves with
// fixed roles: waves 4-7 PRODUCE stages (neighbour indices, gathers, weight tiles, fp32 -> 2 x fp16 split, LDS stores)
// into a ring of NSLOT LDS slots, waves 0-3 CONSUME them (fragment reads + MFMAs) and never execute a load, a conversion
// or a store; the two sides meet only through per-slot counters in LDS (full / empty, monotonic), no s_barrier after
// the prologue.  Same stage order, same products, same sums as the stage kernel: results are bit-identical.
// ================================================================================================================
__device__ __forceinline__ bool ws_wait(const int* cnt, int target) {
  // bounded spin (a lost signal must never hang the GPU): ~0.5 s, then the caller flags the launch as failed
  for (int spin = 0; spin < (1 << 24); ++spin) {
    if (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= target) return true;
    __builtin_amdgcn_s_sleep(1);
  }
  return false;
}

template <int WAVES_M, int WAVES_N, int TM, int TN, bool HAS_RES, int NSLOT, int NWP = 4>
__global__ __launch_bounds__(64 * (WAVES_M * WAVES_N + NWP), (WAVES_M * WAVES_N > 4 ? 3 : (TM * TN >= 4 ? 2 : 4)))
void sparse_conv_ws_kernel(ConvArgs p, const __bf16* __restrict__ wt) {
  constexpr int NWC = WAVES_M * WAVES_N, PT = 64 * NWP, NTHREADS = 64 * (NWC + NWP);      // consumer waves, producer threads
  constexpr int BM = 32 * TM * WAVES_M, BN = 32 * TN * WAVES_N, NP = 2;
  constexpr int A_ITERS = (BM << 3) / PT;
  constexpr int B_CHUNKS = NP * BN * (BK / 8);
  constexpr int B_ITERS = (B_CHUNKS + PT - 1) / PT;
  constexpr int A_ELEMS = NP * BM * LDK, B_ELEMS = NP * BN * LDK, SLOT_ELEMS = A_ELEMS + B_ELEMS;
  static_assert((BM << 3) % PT == 0 && A_ITERS >= 1 && B_ITERS >= 1, "tile shape");
  extern __shared__ __attribute__((aligned(16))) unsigned char ws_lds[];
  __bf16* ring = reinterpret_cast<__bf16*>(ws_lds);                       // [NSLOT][A planes | B planes]
  int* ctl = reinterpret_cast<int*>(ws_lds + (size_t)NSLOT * SLOT_ELEMS * sizeof(__bf16));
  int* full_cnt = ctl;                   // [NSLOT] producer waves that finished writing the slot (monotonic)
  int* empty_cnt = ctl + NSLOT;          // [NSLOT] consumer waves that finished reading it
  unsigned* mask_s = reinterpret_cast<unsigned*>(ctl + 2 * NSLOT);
  int* done_cnt = ctl + 2 * NSLOT + 1;
  float* amax_s = reinterpret_cast<float*>(ctl + 2 * NSLOT + 2);         // [NWC]

  const int64_t n_live = live_rows(p.no_cap, p.no_dev);
  const int64_t tile0 = (int64_t)blockIdx.x * BM;
  if (tile0 >= n_live) return;
  const int cout0 = blockIdx.y * BN;
  const int zs = blockIdx.z;
  const int Cin = p.Cin, Cout = p.Cout, K = p.K;
  const int Cout_p = conv_cout_padded(Cout);
  const int64_t plane_elems = (int64_t)(p.slices > 1 ? p.slices : 1) * (p.tile_tap ? p.w_taps : K) * Cin * Cout_p;
  const __bf16* Wz = wt + (p.slices > 1 ? (int64_t)zs * K * Cin * Cout_p : 0) +
                     (p.tile_tap ? (int64_t)p.tile_tap[tile0 >> 7] * Cin * Cout_p : 0);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const bool producer = wid >= NWC;

  int k_lo = 0, k_hi = K;
  if (p.splits > 1) { k_lo = zs * p.k_per_split; k_hi = min(K, k_lo + p.k_per_split); }
  const int rows_here = (int)min((int64_t)BM, n_live - tile0);
  if (tid < 2 * NSLOT + 2) ctl[tid] = 0;
  __syncthreads();
  if (p.nbr == nullptr) {
    if (tid == 0) *mask_s = 1u;
  } else {
    unsigned local = 0;
    const int32_t* nb = p.nbr + tile0 * K;
    const int kr = k_hi - k_lo;
    for (int i = tid; i < rows_here * kr; i += NTHREADS) {
      const int row = i / kr, k = k_lo + (i - row * kr);
      if (nb[row * K + k] >= 0) local |= 1u << k;
    }
    if (local) atomicOr(mask_s, local);
  }
  __syncthreads();                          // the last block-wide barrier
  const unsigned mask = *mask_s;
  auto next_active = [&](int k) { const unsigned rest = mask & ~((2u << k) - 1u); return rest ? __ffs(rest) - 1 : -1; };

  if (producer) {
    // ---------------------------------------------------------------------------------------------- producers (waves 4-7)
    const int ptid = tid - 64 * NWC;
    const float a_scale = f16_scale_for(read_amax(p.in_amax));
    int32_t src_cur[A_ITERS], src_nxt[A_ITERS];
    auto load_src = [&](int k, int32_t* dst) {
#pragma unroll
      for (int i = 0; i < A_ITERS; ++i) {
        const int row = (ptid + i * PT) >> 3;
        int32_t v = -1;
        if (row < rows_here && k >= 0) v = p.nbr ? p.nbr[(tile0 + row) * K + k] : (int32_t)(tile0 + row);
        dst[i] = v;
      }
    };
    typedef AStageRegs<false, A_ITERS, PT> ARegs;
    ARegs areg;
    u32x4_t rb[B_ITERS];
    auto load_stage = [&](int k, int cin0, const int32_t* srcs) {
      areg.load(p.in, nullptr, 0, ptid, srcs, cin0, 0, Cin);
      const __bf16* Wk = Wz + ((int64_t)k * (Cin / BK) + cin0 / BK) * Cout_p * BK;
#pragma unroll
      for (int i = 0; i < B_ITERS; ++i) {
        int idx = ptid + i * PT;
        idx = idx < B_CHUNKS ? idx : 0;
        const int chunk = idx & 3, row = (idx >> 2) % BN, pl = idx / (4 * BN);
        rb[i] = *reinterpret_cast<const u32x4_t*>(Wk + pl * plane_elems + (int64_t)(cout0 + row) * BK + chunk * 8);
      }
    };
    int k = mask ? __ffs(mask) - 1 : -1;
    int cin0 = 0;
    load_src(k, src_cur);
    load_src(k >= 0 ? next_active(k) : -1, src_nxt);
    if (k >= 0) load_stage(k, 0, src_cur);
    for (int s = 0; k >= 0; ++s) {
      const int slot = s % NSLOT, round = s / NSLOT;
      __bf16* A = ring + (size_t)slot * SLOT_ELEMS;
      __bf16* B = A + A_ELEMS;
      if (round > 0 && !ws_wait(&empty_cnt[slot], NWC * round)) { if (lane == 0) *done_cnt = -1000; return; }
      areg.template store<1>(ptid, A, A + BM * LDK, A + BM * LDK, a_scale);
#pragma unroll
      for (int i = 0; i < B_ITERS; ++i) {
        const int idx = ptid + i * PT;
        if (idx < B_CHUNKS) {
          const int chunk = idx & 3, row = (idx >> 2) % BN, pl = idx / (4 * BN);
          *reinterpret_cast<u32x4_t*>(&B[pl * BN * LDK + lds_slot(row, chunk)]) = rb[i];
        }
      }
      // LDS executes one wave's operations in order: the counter update below lands behind the stores above
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
      if (lane == 0) __hip_atomic_fetch_add(&full_cnt[slot], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
      cin0 += BK;
      if (cin0 >= Cin) {
        cin0 = 0;
        k = next_active(k);
#pragma unroll
        for (int i = 0; i < A_ITERS; ++i) src_cur[i] = src_nxt[i];
        if (k >= 0) load_src(next_active(k), src_nxt);
      }
      if (k >= 0) load_stage(k, cin0, src_cur);
    }
    return;
  }

  // ------------------------------------------------------------------------------------------------ consumers (waves 0-3)
  const int wr = wid / WAVES_N, wc = wid % WAVES_N;
  const float out_scale = 1.0f / (f16_scale_for(read_amax(p.in_amax)) * f16_scale_for(*p.w_amax));
  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.0f;
  const int n_stages = __popc(mask) * (Cin / BK);
  const int a_row = wr * (32 * TM) + (lane & 31), b_row = wc * (32 * TN) + (lane & 31), fhalf = lane >> 5;
  bool ok = true;
  for (int s = 0; s < n_stages; ++s) {
    const int slot = s % NSLOT, round = s / NSLOT;
    const __bf16* A = ring + (size_t)slot * SLOT_ELEMS;
    const __bf16* B = A + A_ELEMS;
    if (!ws_wait(&full_cnt[slot], NWP * (round + 1))) { ok = false; break; }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
#pragma unroll
    for (int ks = 0; ks < BK; ks += 16) {
      f16x8_t af[TM][2], bf[TN][2];
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) af[a][pl] = *reinterpret_cast<const f16x8_t*>(&A[pl * BM * LDK + lds_slot(a_row + a * 32, (ks >> 3) + fhalf)]);
#pragma unroll
      for (int b = 0; b < TN; ++b)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) bf[b][pl] = *reinterpret_cast<const f16x8_t*>(&B[pl * BN * LDK + lds_slot(b_row + b * 32, (ks >> 3) + fhalf)]);
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b) {
          f32x16 c = acc[a][b];
          c = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[a][1], bf[b][0], c, 0, 0, 0);    // m*h
          c = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[a][0], bf[b][1], c, 0, 0, 0);    // h*m
          c = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[a][0], bf[b][0], c, 0, 0, 0);    // h*h
          acc[a][b] = c;
        }
    }
    // the fragment reads have returned (the MFMAs above consumed them): the slot may be overwritten
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    if (lane == 0) __hip_atomic_fetch_add(&empty_cnt[slot], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  if (!ok) return;

  // (as the stage kernel: a split launch sends its sums to its slab through the same chain)
  const bool partial = p.splits > 1;
  const bool use_scale = !partial && p.scale != nullptr, use_shift = !partial && p.shift != nullptr;
  float mx = 0.0f;
  EpiOut o{partial ? p.slab + (int64_t)zs * p.no_cap * Cout : p.out, p.residual, partial ? 0 : p.act, Cout, n_live};
  if (p.slices > 1) { o.row_step = p.slices; o.child = morton_child(zs); }                         // see slice_out_row()
#pragma unroll
  for (int b = 0; b < TN; ++b) {
    const EpiCol c = epi_col(p, cout0 + wc * (32 * TN) + b * 32 + (lane & 31), use_scale, use_shift);
#pragma unroll
    for (int a = 0; a < TM; ++a) {
      epilogue_tile<true, HAS_RES, true>(acc[a][b], tile0 + wr * (32 * TM) + a * 32 + 4 * (lane >> 5), c, out_scale, o, mx);
    }
  }
  if (!partial && p.out_amax != nullptr) {
    // block maximum without a block barrier (the producer waves are gone): the consumer wave that arrives last publishes
    mx = wave_max(mx);
    if (lane == 0) amax_s[wid] = mx;
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    int arrived = 0;
    if (lane == 0) arrived = __hip_atomic_fetch_add(done_cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    arrived = __shfl(arrived, 0, 64);
    if (arrived == NWC - 1 && lane == 0) {
      float m = amax_s[0];
      for (int i = 1; i < NWC; ++i) m = fmaxf(m, amax_s[i]);
      amax_publish_candidate(p.out_amax, m);
    }
  }
}

template <int WM, int WN, int TM_, int TN_, int NSLOT>
int launch_ws_one(bool has_res, dim3 grid, const ConvArgs& p, const __bf16* wt, hipStream_t st) {
  constexpr int BM = 32 * TM_ * WM, BN = 32 * TN_ * WN, NWC = WM * WN, NWP = 4;
  const size_t lds = (size_t)NSLOT * (BM + BN) * LDK * 2 * sizeof(uint16_t) + (2 * NSLOT + 2 + NWC) * sizeof(int);
  if (lds > 160 * 1024) return CNRMA_EINVAL;
  auto go = [&](auto kernel) -> int {
    if (lds > 48 * 1024) {
      static bool raised = false;           // per instantiation (the lambda is instantiated per kernel type)
      if (!raised) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return -(int)e;
        raised = true;
      }
    }
    hipLaunchKernelGGL(kernel, grid, dim3(64 * (NWC + NWP)), lds, st, p, wt);
    return 0;
  };
  return has_res ? go(sparse_conv_ws_kernel<WM, WN, TM_, TN_, true, NSLOT>) : go(sparse_conv_ws_kernel<WM, WN, TM_, TN_, false, NSLOT>);
}

template <int NSLOT>
int launch_ws_shape(int shape, bool has_res, dim3 grid, const ConvArgs& p, const __bf16* wt, hipStream_t st) {
  switch (shape) {
    case 0: return launch_ws_one<2, 2, 2, 2, NSLOT>(has_res, grid, p, wt, st);      // 128x128
    case 1: return launch_ws_one<4, 1, 1, 2, NSLOT>(has_res, grid, p, wt, st);      // 128x64
    case 2: return launch_ws_one<2, 2, 1, 1, NSLOT>(has_res, grid, p, wt, st);      // 64x64
    case 4: return launch_ws_one<2, 2, 1, 2, NSLOT>(has_res, grid, p, wt, st);      // 64x128
    case 5: return launch_ws_one<4, 2, 2, 2, NSLOT>(has_res, grid, p, wt, st);      // 256x128: 8 consumer waves of 64x64
    case 6: return launch_ws_one<4, 2, 2, 1, NSLOT>(has_res, grid, p, wt, st);      // 256x64:  8 consumer waves of 64x32
    default: return CNRMA_EINVAL;
  }
}

int launch_conv_ws(int shape, int slots, bool has_res, dim3 grid, const ConvArgs& p, const __bf16* wt, hipStream_t st) {
  if (slots >= 4 && shape != 0 && shape < 5) return launch_ws_shape<4>(shape, has_res, grid, p, wt, st);
  if (slots >= 3 && (shape < 5 || shape == 6)) return launch_ws_shape<3>(shape, has_res, grid, p, wt, st);
  return launch_ws_shape<2>(shape, has_res, grid, p, wt, st);
}

