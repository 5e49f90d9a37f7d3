// The fused "predictor tail + grouped top-k" row at any predictor length, through a flat 16-bit image of the map in LDS: the body
// of predictor_tail_select_gen_kernel and tail_select_row_gen (sea_topk.hip, which says why it is stamped and not called).
// In scope: T, E, EPT, TAB_LDS; tp (TailParams), p (TopkParams), s_z (the dynamic LDS, TailLds(H, W4, TAB_LDS ? E : 0, 2 H T_m)), row.
  constexpr int R = EPT / 4;
  constexpr int NBC = E >= 6 ? 4 : 8;                             // heads per batch of the tail stage (register budget)
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = row / tp.T, t = row - n * tp.T;
  const TailLds L(tp.H, tp.W4, TAB_LDS ? E : 0);                   // z tile | table (TAB_LDS) | flat image
  const int LDZ = L.ldz;
  uint32_t* s_tab = reinterpret_cast<uint32_t*>(s_z + L.tab);       // (TAB_LDS) per-pixel constants [3][64 E]
  unsigned short* s_flat = reinterpret_cast<unsigned short*>(s_z + L.flat);
  TailRow<T, E> tr;
  if constexpr (!TAB_LDS) tr.load_global(tp.tab, lane);           // (launcher: not null)
  tail_z_tile<T>(tp, s_z, n, t);
  if constexpr (TAB_LDS) tail_consts_fill<T>(tp, s_tab, 64 * E);
  __syncthreads();
  if constexpr (TAB_LDS) tr.load(s_tab, lane);
  const int mine = max(0, (tp.H - wv + 3) / 4);                   // heads wv, wv + 4, ... of this wave
  for (int k0 = 0; k0 < mine; k0 += NBC) {
    float a[NBC][E];
    const int nb = min(NBC, mine - k0);
    tr.heads(tp, lane, nb, [&](int b) { return s_z + (wv + 4 * (k0 + b)) * LDZ; },
             [&](int b) { return (((int64_t)n * tp.H + (wv + 4 * (k0 + b))) * tp.T + t) * tp.T_M; }, a);
#pragma unroll
    for (int b = 0; b < NBC; ++b) {
      if (b < nb) {
        unsigned short* fr = s_flat + (wv + 4 * (k0 + b)) * tp.T_M + lane * E;
#pragma unroll
        for (int e = 0; e < E; ++e)
          if (lane * E + e < tp.T_M) fr[e] = __builtin_bit_cast(unsigned short, from_f<T>(a[b][e]));
      }
    }
  }
  __syncthreads();
  uint32_t key[EPT / 2];                                           // two 16-bit keys per register (select_body, K16)
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int c = j * TK_THREADS + tid;
    uint2 v = make_uint2(0u, 0u);
    if (c < p.nchunks) v = *reinterpret_cast<const uint2*>(s_flat + 4 * c);
    key[2 * j] = v.x;
    key[2 * j + 1] = v.y;
  }
  select_body<T, EPT, false, false, 64, true, true, false>(p, key, 0ull, n, t, row, (const T*)nullptr, reinterpret_cast<uint32_t*>(s_z));
