// prt_shade2_body.inc -- the body of the shading kernels k_shade2<EXT, I0> (prt_shade2.h) and k_shade2d<I0>
// (prt_defer.hip), included inside each: the kernel's parameters S, A, M, B, iter and the constants EXT, I0, DEFER are
// in scope.  Text, not a function: the kernels of prt_wave2.hip keep their machine code to the byte.
  static_assert(!(EXT && I0), "the light-visibility record belongs to the plain pipelines");
  static_assert(!(EXT && DEFER), "the deferred resolve belongs to the plain pipeline");
  const Shade2ArgsPtr args = (Shade2ArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
  if (args->iter != iter || args->B.n != B.n) {  // the layout above does not match this compiler's: fail the call
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(S.diag + 1, 1u);
    return;
  }
  __shared__ uint32_t pref[kNSub + 1];
  __shared__ uint32_t sm[8];
  const uint32_t* q = (iter & 1) ? B.q1 : B.q0;
  uint32_t* qn = (iter & 1) ? B.q0 : B.q1;
  const uint32_t sub = blockIdx.x % kNSub;
  uint32_t* shcnt = qcounter(B.ctr, iter, 1, sub);
  uint32_t* ncnt = qcounter(B.ctr, iter + 1, 0, sub);
  uint32_t* shq = B.shq + (size_t)sub * B.scap;
  const uint32_t total = load_prefix(B.ctr, iter, 0, pref);
  const uint32_t fl = A.flags;
  // software pipeline over the grid-stride chunks: the next chunk's item, info, hit and seed are loaded while this
  // chunk's item is shaded
  uint32_t item_n = 0, info_n = 0, seed_n = 0;
  float4 hh_n = make_float4(kFar, 0.0f, 0.0f, 0.0f);
  float4 ro_n = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rd_n = ro_n;  // (plain form: the ray too)
  uint2 lv_n = make_uint2(0u, 0u);                                 // (I0: the entry's light-visibility bytes)
  auto prefetch = [&](uint32_t cc) {
    const uint32_t gg = cc * kBlock + threadIdx.x;
    if (gg < total) {
      item_n = q[map_slot(pref, gg, B.qcap)];
      info_n = B.info[item_n];
      // iteration 0 with primary-hit reuse (plain form only): the hit of the pixel's fixed path-1 primary ray
      hh_n = (!EXT && iter == 0 && B.pmode != kPrimTrace) ? B.phit[(B.base + item_n) % B.pitems] : B.hit[item_n];
      if constexpr (I0) lv_n = B.lvis[(B.base + item_n) % B.pitems];
      seed_n = B.seed[item_n];
      if (!EXT) { ro_n = B.ro[item_n]; rd_n = B.rd[item_n]; }
    }
  };
  prefetch(blockIdx.x);
  for (uint32_t c = blockIdx.x; c * kBlock < total; c += gridDim.x) {
    const float4 ro_c = ro_n, rd_c = rd_n;
    // The scene and buffer descriptors are read from the kernarg segment inside each chunk (scalar loads, scalar
    // cache) instead of being held in SGPRs across the loop: their ~90 live words spilled to VGPR lanes (378
    // v_readlane in the loop) when hoisted.  The empty asm hides the pointer's loop invariance.
    Shade2ArgsPtr ka = args;
    asm volatile("" : "+s"(ka));
    const SceneDev& Sc = *(const SceneDev*)&ka->S;
    const WaveBufs& Bc = *(const WaveBufs*)&ka->B;
    const uint32_t g = c * kBlock + threadIdx.x;
    uint32_t item = 0, info = 0, seed = 0, nr = 0;
    uint32_t ask = 0, vis0 = 0;  // (I0) the rays to queue, bit 8k = ray k; the visibility word's initial value
    int kind = 0;
    float4 hh = make_float4(kFar, 0.0f, 0.0f, 0.0f);
    const bool active = g < total;
    if (active) {
      item = item_n; info = info_n; hh = hh_n;
      const uint32_t sd = seed_n;
      const uint2 lv = lv_n;
      if ((info & 0x1FFu) == 0) Bc.s1[item].w = hh.x;                                        // r1.hit.t
      if (!EXT && hh.x >= kFar) {  // a miss (:159): the sky radiance (or 0) ends the path (EXT: k_miss2 / k_resmiss2)
        V3 L = v3(0.0f, 0.0f, 0.0f);
        if (fl & kSkybox) {
          const float4 d = EXT ? Bc.rd[item] : rd_c;
          L = sample_sky_call(Sc.sky, Sc.skyw, Sc.skyh, v3(d.x, d.y, d.z));
        }
        Bc.ne[item] = make_float4(L.x, L.y, L.z, 0.0f);
      }
      if (hh.x < kFar) {
        seed = sd;
        kind = nee_kind(fl, seed);                                                           // :198-214
        nr = (uint32_t)nee_rays(kind);
        if constexpr (I0) lvis_split(lv, kind, ask, vis0);
      }
    }
    prefetch(c + gridDim.x);
    // the block's shadow-ray slots, one atomic (I0: of the rays whose answer is not known yet; the known ones are
    // counted, not queued).  Every other form appends behind the NEE block, once it knows which rays are live
    uint32_t s0 = 0, live = 0;  // (!I0) live: the item's light-class shadow rays to queue, bit k = ray k
    if constexpr (I0)
      s0 = block_append_skip(shcnt, (uint32_t)__popc(ask), qcounter(B.ctr, B.lslot, 1, sub), lvis_total(S),
                             nr - (uint32_t)__popc(ask), sm);
    const uint32_t depth = info & 0xFFu, path = (info >> 8) & 1u;
    uint32_t status = kStMiss, emissive = 0;
    bool next = false;
    bool area_ray = false;
    if (nr) {
      const float4 o = EXT ? Bc.ro[item] : ro_c, d = EXT ? Bc.rd[item] : rd_c;
      const V3 D = v3(d.x, d.y, d.z);
      const uint32_t pk = __float_as_uint(hh.w);
      const V3 I = v3(o.x, o.y, o.z) + hh.x * D;                                             // tiny_bvh.h:586
      const V3 V = -D;
      const HitAttr ha = hit_attributes(Sc, hit_inst(Sc, pk), hit_prim(Sc, pk), hh.y, hh.z, (fl & kNormalMap) != 0);
      float4 nk;
      const V3 brdf = nee_lights(Sc, fl, kind, I, V, ha.N, ha.m, seed, nk, [&](int k, uint32_t light) {
        if constexpr (I0) {  // compact slots: the asked rays below k come first
          if (ask & (1u << (8 * k)))
            shq[s0 + (uint32_t)__popc(ask & ((1u << (8 * k)) - 1u))] = (light << 29) | (4u * item + (uint32_t)k);
        }
      });
      // dead rays (!I0): counted, not queued; their visibility bytes keep the "occluded" 0 stored below
      if constexpr (!I0) live = Bc.dead ? nee_live(Sc, fl, kind, nk, brdf, Bc.dead > 1u) : (1u << nr) - 1u;
      // a shadow ray is queued as (light, visibility index) with the item's hit point I stored once: the traversal
      // kernel rebuilds it (shadow_of, the only reader: an item that queues no light-class ray needs none)
      if (I0 || live) Bc.hp[item] = make_float4(I.x, I.y, I.z, 0.0f);
      const V3 e = v3(0.0f, 0.0f, 0.0f) + v3(1.0f, 1.0f, 1.0f) * ha.m.emis;                // :196
      if (e.x != 0.0f || e.y != 0.0f || e.z != 0.0f) {  // otherwise e is +0 and the resolve rebuilds it
        Bc.ne[item] = make_float4(e.x, e.y, e.z, 0.0f);
        emissive = kRiEmissive;
      }
      Bc.nb[item] = make_float4(brdf.x, brdf.y, brdf.z, 0.0f);
      Bc.nk[item] = nk;
      Bc.vis[item] = I0 ? vis0 : 0u;
      status = kStNeeEnd;
      if constexpr (EXT) {
        // area-light sample (2 draws after the light-class NEE draws) at lit, non-delta, non-dielectric hits
        reinterpret_cast<uint8_t*>(Bc.vis)[4 * (size_t)Bc.n + item] = 0;
        if (Sc.area && (fl & kLighted) && ha.kind != kMatDielectric && !delta_lobe(ha.m)) {
          const float xi1 = random_float(seed), xi2 = random_float(seed);
          Ray sr;
          float tmax;
          V3 fa;
          if (area_nee(area_light(Sc), I, ha.N, V, ha.m, xi1, xi2, sr, tmax, fa)) {
            area_ray = true;
            Bc.ao[item] = make_float4(sr.O.x, sr.O.y, sr.O.z, tmax);
            Bc.ad[item] = make_float4(sr.D.x, sr.D.y, sr.D.z, 0.0f);
            Bc.na[item] = make_float4(fa.x, fa.y, fa.z, 0.0f);
          }
        }
      }
      if ((int)depth != A.bounces - 1) {                                                     // :329
        if (EXT && ha.kind == kMatDielectric) {                                              // :331-372
          const Dielectric dl = dielectric_split(I, D, ha.N);
          const size_t e = (size_t)depth * Bc.n + item;
          Bc.dro[e] = make_float4(dl.refr.O.x, dl.refr.O.y, dl.refr.O.z, dl.fresnel);
          Bc.drd[e] = make_float4(dl.refr.D.x, dl.refr.D.y, dl.refr.D.z, 0.0f);
          Bc.T[e] = make_float4(0.0f, 0.0f, 0.0f, kFar);  // w: the continuation is not BRDF-sampled
          const uint32_t bit = 1u << depth, keep = ~(0x01010101u << depth);
          Bc.dst[item] = (Bc.dst[item] & keep) | bit | (dl.has_refr ? 0u : (bit << 24));
          status = kStNeeCont;
          Bc.ro[item] = make_float4(dl.refl.O.x, dl.refl.O.y, dl.refl.O.z, 0.0f);
          Bc.rd[item] = make_float4(dl.refl.D.x, dl.refl.D.y, dl.refl.D.z, 0.0f);
          Bc.info[item] = (depth + 1u) | (path << 8);
          next = true;
        } else {
          V3 dir, thr;
          float bp = 2.0f;
          if (sample_bounce(ha.m, V, ha.N, seed, dir, thr, EXT ? &bp : nullptr)) {           // :376-399
            status = kStNeeCont;
            float pdf = 0.0f;
            if constexpr (EXT)  // MIS density of the sampled direction (kFar: delta lobe or no light sampling)
              pdf = (bp > 1.0f || !Sc.area || !(fl & kLighted)) ? kFar : brdf_pdf(ha.m, ha.N, V, dir, bp);
            Bc.T[DEFER ? (size_t)item : (size_t)depth * Bc.n + item] = make_float4(thr.x, thr.y, thr.z, pdf);
            const Ray nr2 = make_ray(I + dir * kEpsilon, dir);                               // :404
            Bc.ro[item] = make_float4(nr2.O.x, nr2.O.y, nr2.O.z, 0.0f);
            Bc.rd[item] = make_float4(nr2.D.x, nr2.D.y, nr2.D.z, 0.0f);
            Bc.info[item] = (depth + 1u) | (path << 8);
            next = true;
          }
        }
      }
      Bc.seed[item] = seed;
    }
    if constexpr (!I0) {  // only the mask lived across the NEE block: the live rays' slots, the dead ones counted
      const uint32_t nl = (uint32_t)__popc(live);
      s0 = block_append_skip(shcnt, nl, qcounter(B.ctr, B.lslot, 1, sub), dead_total(S), nr - nl, sm);
      queue_live(shq, s0, kind, live, item);
    }
    if constexpr (EXT) {  // the area-light shadow rays of the block, one more append
      const uint32_t a0 = block_append(shcnt, area_ray ? 1u : 0u, sm);
      if (area_ray) shq[a0] = (kLightArea << 29) | item;
    }
    if (active) {
      if (status != kStNeeCont) {
        if (EXT && Sc.has_diel) next = diel_next(Bc, item, depth, path);
        if (!next) next = start_path2(Sc, A, M, Bc, item, path);
      }
      Bc.rinfo[item] = depth | (path << 8) | (status << 16) | ((uint32_t)kind << 20) | (next ? kRiQueued : 0u) | emissive |
                       (EXT ? 0u : kResFresh) | ((I0 && ask) ? kRiLearn : 0u);
    }
    const uint32_t slot = block_append(ncnt, next ? 1u : 0u, sm);
    if (next) qn[sub * Bc.qcap + slot] = item;
  }
