// Experiments (-DCNRMA_EXPERIMENTS only): the FIRST form of the gather-once convolution (round 4) -- the bit-identity reference of
// the second form (tests) -- with its diagnostic (ablation) instantiation and the in-kernel slab reduction that measured 2.5-3.5x
// slower.  Included by sparse.hip inside its anonymous namespace.

// Weight fragments of the gather-once kernel are fetched with explicit instructions and explicit waits: hipcc's own
// s_waitcnt placement put vmcnt(0) in front of every offset's MFMAs (it cannot count loads issued around a loop back-edge), so
// every offset waited for the fragment fetched one step before it -- an L2 round trip per step.  The asm loads are invisible
// to that pass; go_wait4() names the registers it releases, which keeps their uses behind it.  Older outstanding loads never
// invalidate a compiler-placed vmcnt(n) (returns are in order), and inside the offset loop there are no other vector loads.
template <int OFF>
__device__ __forceinline__ void go_load16(u32x4_t& d, const uint16_t* p) {
  asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(d) : "v"(p), "n"(OFF));       // no "memory": see above
}
__device__ __forceinline__ void go_wait0(u32x4_t (&a)[1][2][2], u32x4_t (&b)[1][2][2]) {      // every load has landed
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(a[0][0][0]), "+v"(a[0][0][1]), "+v"(a[0][1][0]), "+v"(a[0][1][1]),
               "+v"(b[0][0][0]), "+v"(b[0][0][1]), "+v"(b[0][1][0]), "+v"(b[0][1][1]));
}
__device__ __forceinline__ void go_wait4(u32x4_t (&b)[1][2][2]) {          // everything but the 4 newest loads has landed
  asm volatile("s_waitcnt vmcnt(4)" : "+v"(b[0][0][0]), "+v"(b[0][0][1]), "+v"(b[0][1][0]), "+v"(b[0][1][1]));
}

// KS = 2 (the 64-column tile): the four waves are 2 column halves x 2 OFFSET halves -- a wave owns all 64 rows x 32 columns for
// every second offset of the group, so that a weight fragment is fetched by exactly one wave of the block and feeds two row
// tiles (with 2 x 2 waves over rows x columns every fragment was fetched twice per block and fed one: the vector-memory
// path, 64 B/clk/CU, carried 16 KB per 192 MFMA cycles); the two partial sums meet in LDS before the epilogue.
template <int WAVES_M, int WAVES_N, int TM, int TN, bool HAS_RES, int KS = 1, bool ABL = false>
__global__ __launch_bounds__(256, 4) void sparse_conv_go_kernel(ConvArgs p, GoArgs g, const uint16_t* __restrict__ wfrag) {
  // ABL: the diagnostic instantiation (cnrma_debug_conv_tuning ablation mask != 0); the product kernel has none of its branches
  // (a branch around a load makes hipcc wait for every load on its own)
  const int abl = ABL ? p.ablate : 0;
  constexpr int BM = 32 * TM * WAVES_M, BN = 32 * TN * WAVES_N;
  static_assert(BM == GO_BM && WAVES_M * WAVES_N * KS == 4, "tile shape");
  static_assert(KS == 1 || (KS == 2 && TM == 2 && TN == 1 && WAVES_M == 1), "offset halves: one wave = 64 rows x 32 columns");
  __shared__ __attribute__((aligned(16))) __bf16 Us[2][(GO_UMAX + 2) * LDK];      // fp16 bit patterns; row GO_UMAX = zeros, GO_UMAX + 1 = dump
  __shared__ uint16_t Ls[GO_BM * 27];
  const int64_t n_live = live_rows(p.no_cap, p.no_dev);
  const int64_t tile = blockIdx.x, tile0 = tile * BM;
  if (tile0 >= n_live) return;
  const int cout0 = blockIdx.y * BN, zs = blockIdx.z;
  const int Cin = p.Cin, Cout = p.Cout;
  const int Cout_p = conv_cout_padded(Cout), nt = Cout_p / 32, ns = Cin / BK;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int kg = wid / (WAVES_M * WAVES_N), w2 = wid % (WAVES_M * WAVES_N);
  const int wr = w2 / WAVES_N, wc = w2 % WAVES_N;
  const float a_scale = f16_scale_for(read_amax(p.in_amax));
  const float out_scale = 1.0f / (a_scale * f16_scale_for(*p.w_amax));
  const int32_t* th = g.hdr + tile * GO_HDR;
  const int32_t* tr = g.rows + tile * GO_ROWS;
  for (int i = tid; i < GO_BM * 27; i += 256) Ls[i] = (abl & 32) ? (uint16_t)(i & 127) : g.lidx[tile * (GO_BM * 27) + i];
  if (tid < 16) {                                            // the zero row of both planes (64 bytes each)
    reinterpret_cast<uint32_t*>(&Us[0][GO_UMAX * LDK])[tid] = 0u;
    reinterpret_cast<uint32_t*>(&Us[1][GO_UMAX * LDK])[tid] = 0u;
  }
  const int n_groups = th[0];
  int s_lo = 0, s_hi = ns;
  if (p.splits > 1) { s_lo = zs * g.slices_per_split; s_hi = min(ns, s_lo + g.slices_per_split); }

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.0f;

  const int a_row0 = wr * (32 * TM) + (lane & 31), fhalf = lane >> 5;
  // B fragments of one (offset, slice): [TN][plane][k-step] x 16 bytes per lane, straight from the fragment-order image
  static_assert(TN == 1, "one 32-column fragment set per wave");
  auto load_b = [&](u32x4_t (&bf)[TN][2][2], int k, int slice) {
    const uint16_t* base = wfrag + (((int64_t)k * ns + slice) * nt + (cout0 >> 5) + wc * TN) * 2048 + lane * 8;
    go_load16<0>(bf[0][0][0], base);                           // [plane][k-step]: 1024 bytes apart
    go_load16<1024>(bf[0][0][1], base);
    go_load16<2048>(bf[0][1][0], base);
    go_load16<3072>(bf[0][1][1], base);
  };
  // A fragments come from LDS one at a time, each read issued BEFORE the MFMAs of the fragment in front of it (two 16-byte
  // registers in rotation): the register budget of four waves per SIMD leaves no room for a k-step's four fragments at once,
  // and with a single register hipcc had every MFMA group wait for its own LDS round trip (8 per offset: ~1000 cycles for 384
  // cycles of MFMAs).  Order per k-step and row tile: the low plane (one product), then the high plane (two products).
  auto mfma_k = [&](const u32x4_t (&bf)[TN][2][2], int k) {
    int li[TM];
#pragma unroll
    for (int a = 0; a < TM; ++a) li[a] = Ls[(a_row0 + a * 32) * 27 + k];
    auto rd = [&](int a, int pl, int ks) -> f16x8_t {
      return *reinterpret_cast<const f16x8_t*>(&Us[pl][lds_slot(li[a], ks * 2 + fhalf)]);
    };
    f16x8_t cur = rd(0, 1, 0);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const f16x8_t bh = __builtin_bit_cast(f16x8_t, bf[0][0][ks]), bm = __builtin_bit_cast(f16x8_t, bf[0][1][ks]);
#pragma unroll
      for (int a = 0; a < TM; ++a) {
        f16x8_t nxt = rd(a, 0, ks);                                              // this row tile's high plane
        acc[a][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur, bh, acc[a][0], 0, 0, 0);       // m*h
        cur = nxt;
        const bool last = ks == 1 && a == TM - 1;
        if (!last) nxt = a + 1 < TM ? rd(a + 1, 1, ks) : rd(0, 1, ks + 1);       // the next low plane
        acc[a][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur, bm, acc[a][0], 0, 0, 0);       // h*m
        acc[a][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur, bh, acc[a][0], 0, 0, 0);       // h*h
        cur = nxt;
      }
    }
  };

  for (int slice = s_lo; slice < s_hi; ++slice) {
    const int cin0 = slice * BK;
    for (int grp = 0; grp < n_groups; ++grp) {
      const unsigned mask = (unsigned)th[1 + 3 * grp];
      const int ub = th[2 + 3 * grp], un = th[3 + 3 * grp];
      unsigned mymask = mask;
      if constexpr (KS == 2) {                               // every second offset of the group
        mymask = 0;
        unsigned m = mask;
        int r = 0;
        while (m) {
          const unsigned low = m & (0u - m);
          if ((r & 1) == kg) mymask |= low;
          m ^= low;
          ++r;
        }
      }
      // two offsets' weights in flight, in a pattern the compiler can count: EVERY step issues exactly one offset's four loads,
      // unconditionally (behind the last offset the last one again), so the wait in front of an offset's MFMAs is "all but
      // the four newest loads" -- with conditional prefetches hipcc emitted s_waitcnt vmcnt(0) there and every offset waited
      // for the weights fetched one step before it (an L2 round trip per step: 0.75 us for 0.18 us of MFMAs)
      u32x4_t b0[TN][2][2], b1[TN][2][2];
      unsigned rest = mymask;
      const int n_off = __popc(mymask);
      int k_last = 0;
      auto pop = [&]() { if (rest) { k_last = __ffs(rest) - 1; rest &= rest - 1u; } return k_last; };
      int k0 = pop(), k1 = pop();
      load_b(b0, k0, slice);
      load_b(b1, k1, slice);
      __syncthreads();                                       // the previous stage's fragment reads are done
      // ---- the union rows of this group, once: 8 lanes per row (4 channels each), 4 rows per thread in flight (more in
      // flight, or the row numbers of all batches up front, costs the third wave per SIMD: measured 20-35 % slower)
      const int tasks = un * 8;
      for (int t0 = 0; t0 < tasks; t0 += 256 * 4) {
        float4 v[4];
        int32_t src[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {                          // the four row numbers first, then the four rows: two round trips
          const int t = t0 + i * 256 + tid;                    // per batch instead of up to eight
          src[i] = tr[ub + (t < tasks ? (t >> 3) : 0)];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int t = t0 + i * 256 + tid;
          if (!(abl & 2)) v[i] = *reinterpret_cast<const float4*>(p.in + (int64_t)src[i] * Cin + cin0 + (t & 7) * 4);
          else v[i] = make_float4(0.f, 0.f, 0.f, (float)src[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          // EVERY loaded value is consumed here, on every path (tasks behind the union go to a dump row): a load whose use
          // sits behind a branch stays "pending" for hipcc's wait placement, and the wait for it lands in the header of the
          // offset loop below -- where it would drain the weight prefetches on every iteration
          const int t = t0 + i * 256 + tid;
          const int u = t < tasks ? (t >> 3) : GO_UMAX + 1, kc = t & 7;
          uint2 h, m;
          split2(v[i], a_scale, h, m);
          const int o = lds_slot(u, kc >> 1) + (kc & 1) * 4;
          if (!(abl & 8)) {
            *reinterpret_cast<uint2*>(&Us[0][o]) = h;
            *reinterpret_cast<uint2*>(&Us[1][o]) = m;
          } else if (h.x == 0x12345678u) Us[0][0] = (__bf16)0.0f;
        }
      }
      __syncthreads();
      // ---- the group's offsets back to back: no barrier, no LDS store, no index load from memory
      int i = 0;
      for (; i + 2 < n_off; i += 2) {                          // steady state: two offsets per turn, their successors prefetched
        go_wait4(b0);                                          // b0 has landed; b1's four loads may still fly
        if (!(abl & 1)) mfma_k(b0, k0);
        k0 = pop();
        load_b(b0, k0, slice);
        go_wait4(b1);                                          // b1 has landed; the four just issued may fly
        if (!(abl & 1)) mfma_k(b1, k1);
        k1 = pop();                                            // behind the last offset: the last one again (never used)
        load_b(b1, k1, slice);
      }
      // the last one or two offsets: nothing more to prefetch, and NO load may be left in flight -- the asm loads are invisible
      // to the compiler, which is free to reuse their destination registers from here on
      go_wait0(b0, b1);
      if (i < n_off && !(abl & 1)) mfma_k(b0, k0);
      if (i + 1 < n_off && !(abl & 1)) mfma_k(b1, k1);
    }
  }

  // (the images are dead: 4 x 4 KB of the 20-KB plane)
  if constexpr (KS == 2) merge_offset_halves(acc[0][0], acc[1][0], reinterpret_cast<float*>(&Us[0][0]), wc, kg, lane);

  // ---- epilogue (as the stage kernel).  Split over channel slices: every block leaves its partial tile in its slab; with a
  // counter array (g.counters, zero between launches) the LAST block of a tile to arrive adds the slabs up in slab order --
  // the sums conv_reduce_kernel forms, bit for bit -- and finishes the tile itself: no reduce launch behind the kernel.
  // The partial tiles cross XCDs inside one kernel: they are written and read with device-scope accesses, and a release /
  // acquire fence pair stands around the counter.
  float oscale = out_scale;
  if (p.splits > 1) {
    float* slab = p.slab + (int64_t)zs * p.no_cap * Cout;
    const bool here = g.counters != nullptr;
#pragma unroll
    for (int b = 0; b < TN; ++b) {
      const int col = cout0 + wc * (32 * TN) + b * 32 + (lane & 31);
#pragma unroll
      for (int a = 0; a < TM; ++a) {
        if (KS == 2 && a != kg) continue;
        const int64_t row0 = tile0 + wr * (32 * TM) + a * 32 + 4 * (lane >> 5);
        slab_tile<true>(acc[a][b], row0, col, col < Cout, out_scale, slab, Cout, n_live);
      }
    }
    if (!here) return;                                       // conv_reduce_kernel follows
    __shared__ int s_last;
    __threadfence();
    __syncthreads();
    if (tid == 0) {
      unsigned* c = g.counters + (blockIdx.x * gridDim.y + blockIdx.y);
      const unsigned old = atomicAdd(c, 1u);
      s_last = old == (unsigned)p.splits - 1u;
      if (s_last) __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    const int64_t slab_stride = p.no_cap * Cout;
#pragma unroll
    for (int b = 0; b < TN; ++b) {
      const int col = cout0 + wc * (32 * TN) + b * 32 + (lane & 31);
#pragma unroll
      for (int a = 0; a < TM; ++a) {
        if (KS == 2 && a != kg) continue;
        const int64_t row0 = tile0 + wr * (32 * TM) + a * 32 + 4 * (lane >> 5);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int64_t row = row0 + (i & 3) + 8 * (i >> 2);
          float sum = 0.0f;
          if (col < Cout && row < n_live) {
            const float* q = p.slab + row * Cout + col;
            sum = __builtin_nontemporal_load(q);
            for (int z = 1; z < p.splits; ++z) sum += __builtin_nontemporal_load(q + (int64_t)z * slab_stride);
          }
          acc[a][b][i] = sum;
        }
      }
    }
    oscale = 1.0f;                                           // the slabs hold scaled sums
  }
  const bool has_res_rt = !HAS_RES && p.residual != nullptr;  // a split launch is instantiated without the residual template
  float mx = 0.0f;
  const EpiOut o{p.out, p.residual, p.act, Cout, n_live};
  // ablation bit 4: no stores, behind a test on the value that keeps the arithmetic alive
  auto keep = [=](float v) { return !((abl & 16) && v != 12345.678f); };
  auto finish = [&](auto with_res) {
#pragma unroll
    for (int b = 0; b < TN; ++b) {
      const EpiCol c = epi_col(p, cout0 + wc * (32 * TN) + b * 32 + (lane & 31), p.scale != nullptr, p.shift != nullptr);
#pragma unroll
      for (int a = 0; a < TM; ++a) {
        if (KS == 2 && a != kg) continue;
        epilogue_tile<true, decltype(with_res)::value, true>(acc[a][b], tile0 + wr * (32 * TM) + a * 32 + 4 * (lane >> 5), c, oscale,
                                                             o, mx, keep);
      }
    }
  };
  if (has_res_rt) finish(std::true_type{});                  // the one runtime residual: one branch per block, outside the tile loops
  else finish(std::integral_constant<bool, HAS_RES>{});
  if (p.out_amax != nullptr) {
    __syncthreads();
    block_amax_publish(p.out_amax, mx, reinterpret_cast<float*>(&Us[0][0]));
  }
}


// the first form's launcher (p, g: the layer as cnrma_sparse_conv_go_f16x3 prepared it).  Short layers: split over the 32-channel
// slices (every block still runs all 27 offsets of its slices); the partial slabs are reduced by conv_reduce_kernel in a fixed
// order, or in the kernel when arrival counters are handed over
static int launch_go1(ConvArgs p, GoArgs g, const uint16_t* wfrag, size_t workspace_bytes, void* tile_counters, hipStream_t st) {
  const int64_t no_cap = p.no_cap, tiles = ceil_div(no_cap, GO_BM);
  const int Cout = p.Cout, bn = Cout >= 128 ? 128 : 64, ns = p.Cin / BK;
  int splits = 1;
  const int64_t blocks = tiles * ceil_div(Cout, bn);
  const int force = CNRMA_CONV_TUNE.splits;
  if (p.slab != nullptr && ns > 1 && (blocks < 384 || force > 0)) {
    splits = force > 0 ? force : (int)ceil_div(768, blocks);
    if (splits > ns) splits = ns;
    const size_t per = (size_t)no_cap * Cout * sizeof(float);
    if (per > 0 && (size_t)splits * per > workspace_bytes) splits = (int)(workspace_bytes / per);
    if (splits < 2) splits = 1;
  }
  g.slices_per_split = (int)ceil_div(ns, splits);
  splits = (int)ceil_div(ns, g.slices_per_split);
  p.splits = splits;
  g.counters = splits > 1 ? reinterpret_cast<unsigned*>(tile_counters) : nullptr;
  const bool has_res = p.residual != nullptr && splits == 1;
  dim3 grid((unsigned)tiles, (unsigned)ceil_div(Cout, bn), (unsigned)splits);
  if (p.ablate != 0 && !has_res) {                         // diagnostic instantiations (timing experiments only)
    if (bn == 128) hipLaunchKernelGGL((sparse_conv_go_kernel<1, 4, 2, 1, false, 1, true>), grid, dim3(256), 0, st, p, g, wfrag);
    else hipLaunchKernelGGL((sparse_conv_go_kernel<1, 2, 2, 1, false, 2, true>), grid, dim3(256), 0, st, p, g, wfrag);
  } else if (bn == 128) {
    if (has_res) hipLaunchKernelGGL((sparse_conv_go_kernel<1, 4, 2, 1, true>), grid, dim3(256), 0, st, p, g, wfrag);
    else hipLaunchKernelGGL((sparse_conv_go_kernel<1, 4, 2, 1, false>), grid, dim3(256), 0, st, p, g, wfrag);
  } else {
    if (CNRMA_CONV_TUNE.pf == 3) {                             // A/B aid: the 2 x 2 waves-over-rows-x-columns form
      if (has_res) hipLaunchKernelGGL((sparse_conv_go_kernel<2, 2, 1, 1, true>), grid, dim3(256), 0, st, p, g, wfrag);
      else hipLaunchKernelGGL((sparse_conv_go_kernel<2, 2, 1, 1, false>), grid, dim3(256), 0, st, p, g, wfrag);
    } else if (has_res) hipLaunchKernelGGL((sparse_conv_go_kernel<1, 2, 2, 1, true, 2>), grid, dim3(256), 0, st, p, g, wfrag);
    else hipLaunchKernelGGL((sparse_conv_go_kernel<1, 2, 2, 1, false, 2>), grid, dim3(256), 0, st, p, g, wfrag);
  }
  if (g.counters == nullptr) reduce_splits(p, st);
  CNRMA_LAUNCH_CHECK();
  return 0;
}
