// The body of K2's kernels (pgp_encoder.hip), included into encoder_kernel<H, SPLIT>
// and encoder_asplit_kernel<H>: kernels of their own names that share every
// statement.  In scope at the point of inclusion: H, SPLIT, AS (constants), the
// kernel's argument `a`, L = EncLds<H, SPLIT, AS> and its __shared__ arrays
// smem[L::TOTAL] (weights | tables; AS: tables | weights) and xstage (the tail-resident mode's
// per-wave staging slots of the next unit's raw features).
  using G = Geo<H>;
  // AS: the tables first, so that every table read is lane-group base + immediate (the weights' reads
  // re-derive their lane offset at each use anyway): no table address held in a VGPR across the unit loop
  float* tab = smem + (AS ? 0 : L::RESIDENT ? L::STREAM : 2 * L::SLOT);
  const int tsz = G::t_size(a.K);
  for (int i = threadIdx.x; i < tsz; i += blockDim.x) tab[i] = a.tab[i];

  const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr int NW = enc_waves<H>();
  const long nblk = (a.B + 15) / 16;

  Ring<H, SPLIT, AS> ring{smem, smem + L::SLOT, a.frags + G::OFF_ENC, 0, H * kLayers * G::NST, wv, lane};
  if constexpr (AS) {
    ring.enc = a.encb + EncS<H>::SIZE;  // the EncA image: its first RES_G groups to LDS, the rest read per unit
    dma_groups(ring.enc, smem + L::TAB, EncA<H>::RES_G, wv, NW, lane);
    ring.nxt = smem + L::TAB;
    ring.next = 1;
    __syncthreads();
  } else if constexpr (SPLIT) {
    dma_groups(a.encb, smem, EncS<H>::GROUPS, wv, NW, lane);
    ring.nxt = smem;
    ring.next = 1;
    __syncthreads();
  } else if constexpr (L::RESIDENT) {
    dma_groups(a.frags + G::OFF_ENC + (long)L::RES0 * G::FQ, smem, kLayers * G::LAYER_G - L::RES0, wv, NW, lane);
    ring.nxt = smem;
    ring.next = 1;
    __syncthreads();
  } else {
    ring.nxt = smem;  // prologue: stage 0 -> slot 0
    ring.issue();
    ring.nxt = smem + L::SLOT;
    ring.next = 1;
    __syncthreads();
    ring.issue();  // stage 1 -> slot 1
  }

  // one (16-window block, host) unit: hosts are independent in the encoder
  // one (16-window block, host) unit: hosts are independent in the encoder.
  // tail-resident mode: pre = the unit's 144 raw-feature floats ([step][feature]
  // [window], the agg layout) staged in LDS by the caller; otherwise loaded here
  auto unit = [&](long blk, int h, bool active, const float* pre) {
    const float* agg = a.agg + (active ? blk : 0) * H * 3 * 48;
    float* lat = a.lat + (active ? blk : 0) * G::LAT_BLK;
    float ba[3];
    // all 3 raw features of every step of this lane's window (layer 0's bilinear scores)
    float xv[3][3];
    if constexpr (L::UNITS) {
#pragma unroll
      for (int w = 0; w < 3; ++w) {
#pragma unroll
        for (int f = 0; f < 3; ++f) xv[w][f] = G::TAIL ? pre[w * 48 + 16 * f + j] : 0.f;
        const float v = pre[w * 48 + (lane < 48 ? lane : 47)];
        ba[w] = g < 3 ? v : 0.f;  // feature g of window j
      }
    } else {
#pragma unroll
      for (int w = 0; w < 3; ++w) ba[w] = (active && g < 3) ? agg[(h * 3 + w) * 48 + lane] : 0.f;
#pragma unroll
      for (int w = 0; w < 3; ++w)
#pragma unroll
        for (int f = 0; f < 3; ++f)
          xv[w][f] = (G::TAIL && active) ? agg[(h * 3 + w) * 48 + 16 * f + j] : 0.f;
    }
    f32x4 X[G::MT_D][3];
#pragma unroll
    for (int mt = 0; mt < G::MT_D; ++mt) {
      const float aw = tab[G::T_TEW + mt * 64 + lane];
#pragma unroll
      for (int w = 0; w < 3; ++w) X[mt][w] = mfma(aw, ba[w], ld4(tab + G::T_TE + w * G::DP + 16 * mt + 4 * g));
    }
    static_assert(kLayers == 2, "layer 0 (folded q/k/v) + layer 1");
    if constexpr (G::TAIL) {
      encoder_layer_tail<H, true, SPLIT, AS>(X, ring, tab + G::T_L0, lane, tab, ba, xv);
      encoder_layer_tail<H, false, SPLIT, AS>(X, ring, tab + G::T_L0 + G::TL_SIZE, lane, tab, ba, xv);
    } else if constexpr (!SPLIT) {
      encoder_layer<H, true>(X, ring, tab + G::T_L0, lane, tab, ba);
      encoder_layer<H, false>(X, ring, tab + G::T_L0 + G::TL_SIZE, lane, tab, ba);
    }

    if (active) {
#pragma unroll
      for (int w = 0; w < 3; ++w) {
        // chunk (h, w): full groups of 4 k-steps as one 16-byte store per lane,
        // the remaining k-steps one dword each (pgp_layout.hpp, LAT_FG)
        float* lc = lat + (long)((h * 3 + w) * G::KS_D) * 64;
#pragma unroll
        for (int q = 0; q < G::LAT_FG; ++q) *reinterpret_cast<f32x4*>(lc + q * 256 + lane * 4) = X[q][w];
        if constexpr (G::KS_D % 4 != 0) {
#pragma unroll
          for (int r = 0; r < G::KS_D % 4; ++r) lc[G::LAT_FG * 256 + r * 64 + lane] = X[G::LAT_FG][w][r];
        }
      }
      if (a.latent != nullptr) {
        // AS: the tap's lane terms re-derived here (the kernel has no register to keep its addresses
        // across the unit loop; they were its only spills)
        int jt = j, gt = g;
        if constexpr (AS) asm volatile("" : "+v"(jt), "+v"(gt));
        const long b = blk * 16 + jt;
        if (b < a.B) {
#pragma unroll
          for (int w = 0; w < 3; ++w)
#pragma unroll
            for (int mt = 0; mt < G::MT_D; ++mt)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int c = 16 * mt + 4 * r + gt;
                const float* TL1 = tab + G::T_L0 + G::TL_SIZE;  // the latent = gamma * x-hat + beta
                if (c < H)
                  a.latent[b * G::LAT + (long)h * 3 * H + w * H + c] =
                      X[mt][w][r] * TL1[G::TL_LN2G + 16 * mt + 4 * gt + r] + TL1[G::TL_LN2B + 16 * mt + 4 * gt + r];
              }
        }
      }
    }
  };
  if constexpr (L::UNITS) {
    // no barrier in the host loop: each wave takes an equal contiguous range of
    // the nblk x H units (grid = the workgroups that fit at once: CU count x
    // occupancy), so the launch has no partial last round of workgroups
    const long U = nblk * H, NWT = (long)gridDim.x * NW, gw = (long)blockIdx.x * NW + wv;
    const long u1 = (gw + 1) * U / NWT;
    // unit u's raw features are agg[u * 144 ..] (144 floats).  The next unit's
    // are loaded while this one computes and staged through a per-wave LDS slot
    // after this unit's latent stores: no loop-carried registers, so the wait
    // for them is a counted vmcnt in the body (long satisfied) instead of a
    // vmcnt(0) at the loop head that would also wait for the stores.
    float* slot = xstage + wv * 144;
    const long u0 = gw * U / NWT;
    float pf[3];
    auto load_x = [&](long u) {
#pragma unroll
      for (int k = 0; k < 3; ++k) pf[k] = a.agg[u * 144 + (64 * k + lane < 144 ? 64 * k + lane : 143)];
    };
    auto stage_x = [&]() {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (64 * k + lane < 144) slot[64 * k + lane] = pf[k];
    };
    if (u0 < u1) {
      load_x(u0);
      stage_x();
    }
#pragma unroll 1
    for (long u = u0; u < u1; ++u) {
      load_x(u + 1 < u1 ? u + 1 : u);
      const long blk = u / H;
      unit(blk, (int)(u - blk * H), true, slot);
      stage_x();
    }
  } else {
    const long blk = (long)blockIdx.x * NW + wv;
    const bool active = blk < nblk;  // inactive waves still take part in the ring and barriers
#pragma unroll 1
    for (int h = 0; h < H; ++h) unit(blk, h, active, nullptr);
  }
