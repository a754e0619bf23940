// third form (experimental until measured everywhere): persistent grid, two blocks per CU
template <int WAVES_N, int KS, bool HAS_RES, bool STAMP = false>
static int launch_go3_one(unsigned blocks, const ConvArgs& p, const GoArgs& g, const uint16_t* wfrag, const Go3Map& mp, hipStream_t st) {
  auto kernel = sparse_conv_go3_kernel<WAVES_N, KS, HAS_RES, STAMP>;
  static bool raised = false;               // per instantiation: dynamic LDS above the 64-KB default
  if (!raised) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, GO3_LDS);
    if (e != hipSuccess) return -(int)e;
    raised = true;
  }
  if (g_conv_tune.pf == 8) {                               // A/B aid: how many of these blocks a CU holds
    int nb = -1;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(kernel), 256, GO3_LDS);
    fprintf(stderr, "sparse_conv_go3_kernel<%d, %d, %d>: %d blocks per CU at %d bytes of LDS\n", WAVES_N, KS, (int)HAS_RES, nb, GO3_LDS);
  }
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), GO3_LDS, st, p, g, wfrag, mp);
  return 0;
}

static int launch_go3(const Go2Plan& pl, ConvArgs p, GoArgs g, const uint16_t* wfrag, bool residual, void* stamps, hipStream_t st) {
  Go3Map mp;
  mp.tiles = pl.mp.tiles; mp.ncol = pl.mp.ncol; mp.ng = pl.mp.ng;
  mp.n_items = mp.tiles * mp.ng;
  mp.per_xcd = (int)ceil_div(mp.n_items, 8);
  mp.bpx = mp.per_xcd < 64 ? mp.per_xcd : 64;               // 2 blocks x 32 CUs per XCD
  mp.flags = g_conv_tune.pf == 7 ? 1 : 0;
  g.slices_per_split = pl.slices_per_split;
  p.splits = pl.splits;
  g.counters = reinterpret_cast<unsigned*>(stamps);
  const unsigned blocks = 8u * (unsigned)mp.bpx;
  const bool has_res = residual && pl.splits == 1;
  int rc;
  if (stamps != nullptr && !has_res)
    rc = pl.bn == 128 ? launch_go3_one<4, 1, false, true>(blocks, p, g, wfrag, mp, st) : launch_go3_one<2, 2, false, true>(blocks, p, g, wfrag, mp, st);
  else if (pl.bn == 128) rc = has_res ? launch_go3_one<4, 1, true>(blocks, p, g, wfrag, mp, st) : launch_go3_one<4, 1, false>(blocks, p, g, wfrag, mp, st);
  else rc = has_res ? launch_go3_one<2, 2, true>(blocks, p, g, wfrag, mp, st) : launch_go3_one<2, 2, false>(blocks, p, g, wfrag, mp, st);
  if (rc != 0) return rc;
  reduce_splits(p, st);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

// cnrma_sparse_conv_go_f16x3 in the experiments library: the form cnrma_debug_conv_tuning selects (third, second or first); the
// ablation masks other than the stamps (64) exist in the first form only
static int launch_go_experiments(const Go2Plan& pl, const ConvArgs& p, const GoArgs& g, const uint16_t* wfrag, size_t workspace_bytes,
                                 void* tile_counters, hipStream_t st) {
  const bool plain = (p.ablate & ~64) == 0;
  void* stamps = (p.ablate & 64) ? tile_counters : nullptr;
  if (pl.form >= 2 && plain && (uint64_t)p.no_cap * (uint64_t)p.Cin * 4u < (1ull << 32))
    return launch_go3(pl, p, g, wfrag, p.residual != nullptr, stamps, st);
  if (pl.form >= 1 && plain) return launch_go2(pl, p, g, wfrag, p.residual != nullptr, stamps, st);
  return launch_go1(p, g, wfrag, workspace_bytes, tile_counters, st);
}

