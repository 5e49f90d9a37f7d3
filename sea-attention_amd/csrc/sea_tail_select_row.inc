// The fused "predictor tail + grouped top-k" row at T_m = 256, the map in registers: the body of predictor_tail_select_kernel,
// predictor_tail_select_f32_kernel and tail_select_row (sea_topk.hip, which says why it is stamped and not called).
// In scope: T, EPT, FULL; tp (TailParams), p (TopkParams), s_z (the dynamic LDS, TailLds(H, 64, 4)), row.
  constexpr int R = EPT / 4, E = 4;
  constexpr bool K16 = sizeof(T) == 2;                             // two 16-bit keys per register (select_body, K16)
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = row / tp.T, t = row - n * tp.T;
  constexpr int LDZ = TailLds(0, 64, E).ldz;   // W4 == 64 (sea_predictor_tail_select checks): z-row offsets become immediates
#ifdef SEA_STAMP
  unsigned long long _tprev = __builtin_amdgcn_s_memtime();
#endif
  uint32_t* s_tab = reinterpret_cast<uint32_t*>(s_z + TailLds::z_words(tp.H, 64));   // per-pixel constants [3][64 E]
  TailRow<T, E> tr;
  if (tp.tab) tr.load_global(tp.tab, lane);                        // (block-uniform) the table was computed once per weight set
  tail_z_tile<T>(tp, s_z, n, t);
  if (!tp.tab) tail_consts_fill<T>(tp, s_tab, 64 * E);
  __syncthreads();
  if (!tp.tab) tr.load(s_tab, lane);
  STAMP(8);   // z tile (MFMA) + per-pixel constants
  uint32_t key[K16 ? EPT / 2 : EPT];
  const int mine = FULL ? R : max(0, (tp.H - wv + 3) / 4);         // heads wv, wv + 4, ... of this wave (wave-uniform)
  auto batch = [&](auto j0c, auto nbc) {                           // heads 4 (J0 + b) + wv, b < NBC, through one batch
    constexpr int J0 = decltype(j0c)::value, NBC = decltype(nbc)::value;
    float a[NBC][E];
    const int nb = min(NBC, mine - J0);
    if (nb > 0) {
      // T_M == 256 == 64 E here (sea_predictor_tail_select checks): the full-row form, without its ragged twin in the kernel
      tr.template heads_impl<true>(tp, lane, nb, [&](int b) { return s_z + (4 * (J0 + b) + wv) * LDZ; },
                                   [&](int b) { return (((int64_t)n * tp.H + (4 * (J0 + b) + wv)) * tp.T + t) * (64 * E); }, a);
    }
#pragma unroll
    for (int b = 0; b < NBC; ++b) {  // probabilities are >= +0: the 16-bit pattern the map stores orders like the number
      if constexpr (K16) {
        key[2 * (J0 + b)] = (b < nb) ? pack2<T>(a[b][0], a[b][1]) : 0u;
        key[2 * (J0 + b) + 1] = (b < nb) ? pack2<T>(a[b][2], a[b][3]) : 0u;
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) key[4 * (J0 + b) + e] = (b < nb) ? f2key(a[b][e]) : 0u;
      }
    }
  };
  static_assert(R <= 16, "two batches of eight heads per wave");
  if constexpr (R <= 8) {
    batch(std::integral_constant<int, 0>{}, std::integral_constant<int, R>{});
  } else {
    batch(std::integral_constant<int, 0>{}, std::integral_constant<int, 8>{});
    batch(std::integral_constant<int, 8>{}, std::integral_constant<int, R - 8>{});
  }
  STAMP(9);   // 8 heads per wave: resize + LayerNorm + softmax + store
  // H <= 64: sea_predictor_tail_select checks.  The z tile and the constants table are dead once every wave has left the head
  // loop, i.e. from select_body's first barrier on: the candidate list lives there (TailLds sizes the dynamic LDS for both).
  if constexpr (K16) {
    // The packed-key selection never re-reads the map (its slow path works on the registers too): tp.probs may be null.
    select_body<T, EPT, false, FULL, 64, true, true>(p, key, 0ull, n, t, row, (const T*)nullptr, reinterpret_cast<uint32_t*>(s_z));
  } else {
    const T* base = reinterpret_cast<const T*>(tp.probs) + (int64_t)n * p.sn + (int64_t)t * p.st;
    select_body<T, EPT, false, FULL, 64, true, false, false>(p, key, 0ull, n, t, row, base, reinterpret_cast<uint32_t*>(s_z));
  }
