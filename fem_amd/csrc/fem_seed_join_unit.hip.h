// fem_seed_join_unit.hip.h — the middle part of one (strand, group) unit of join_read (fem_seed_join.hip.h): the unit's lists ->
// the flagged values of its group, the bitmap clean again.  Not a header of its own: join_read includes it TWICE, inside its unit
// loop, with FEM_JOIN_UNIT_PLAIN true (no list of the unit has a second chunk, no first chunk holds a remapped entry: long_lists
// and remap are compile-time false, everything about second chunks and the rare path is gone from that copy) and false (the
// general code).  Two copies of the text, so that the two bodies share no register, no branch and no join.  (hv[] is still
// declared in the plain copy; nothing reads or writes it there beyond its dead initialisation.)
//
// Why text and not a function: as a generic lambda `[&](auto plain_c)` the same code compiled to 50-140 bytes of scratch at the
// kernel's 72 registers, with the split switched off as well (docs/NOTEBOOK.md, round 6).  A `template <bool> __device__
// __forceinline__` function taking these names as parameters has NOT been tried.
//
// What the text expects from join_read at the place of inclusion:
//   template parameters / constants  R, BANKED, PADDED, kOptSent, kOptLong, kOptHit, kOptOnce, kOptNoMask, kFlagCap, kWords, kNearTop
//   the unit                         u, f[R], st[R], f_max, keep_all, val[R] (first chunks, raw; changed here), flg_g, n_flag (out)
//   the read / the wave              p, ln, lane4, e, seq_base, sent_a, sent_b, bitmap
//   helpers                          run_base, insert, insert_plain, mark, window_top, LdsWord
// and that `return false` leaves join_read (more flagged values than the group's array takes: the read goes to the generic kernel).
#ifndef FEM_JOIN_UNIT_PLAIN
#error "fem_seed_join_unit.hip.h is a part of join_read (fem_seed_join.hip.h): define FEM_JOIN_UNIT_PLAIN true or false and include it there"
#endif
      constexpr bool kPlain = FEM_JOIN_UNIT_PLAIN;
      const bool long_lists = !kPlain && f_max > (uint32_t)kWave;  // some list has a second chunk (entries 64..127)
      uint32_t hv[R];
#pragma unroll
      for (int t = 0; t < R; ++t) hv[t] = kDenseSent;
      if (long_lists) {
#pragma unroll
        for (int t = 0; t < R; ++t) {
          if (kOptLong && f[t] <= (uint32_t)kWave) continue;  // (wave-uniform: only the runs that have a second chunk)
          const uint32_t last4 = f[t] > (uint32_t)kWave ? (f[t] - 1u) * 4u : 0u;
          const uint32_t at4 = lane4 + 4u * (uint32_t)kWave;
          if (PADDED)
            hv[t] = *(const __attribute__((address_space(1))) uint32_t *)(run_base(u * R + t) + at4);
          else
            hv[t] = *(const __attribute__((address_space(1))) uint32_t *)(run_base(u * R + t) + (at4 < last4 ? at4 : last4));
        }
      }
      bool remap = false;
      if (!kPlain) {
        uint32_t raw_max = val[0];  // (a lane behind a list's end holds the list's last entry: one compare for the unit)
#pragma unroll
        for (int t = 1; t < R; ++t) raw_max = val[t] > raw_max ? val[t] : raw_max;
        if (long_lists) {
#pragma unroll
          for (int t = 0; t < R; ++t) raw_max = hv[t] > raw_max ? hv[t] : raw_max;  // (kDenseSent < kDenseRemap: a run without a second chunk says nothing)
        }
        remap = __builtin_amdgcn_ballot_w64(raw_max >= kDenseRemap) != 0;
      }
      uint32_t max_u = 0;
      bool any_u = true;
      uint64_t vm[R];  // lanes that hold an entry of run t's first chunk (kOptSent): scalar arithmetic on the run's length
#pragma unroll
      for (int t = 0; t < R; ++t) vm[t] = 0;
      if (__builtin_expect(remap, 0)) {
        // rare: entries within kDenseNear of a sequence start are resolved exactly (pos >= start or dropped); the maximum
        // of U then comes from a wave reduction (a dropped entry may sit at the end of a run)
        uint32_t mx = 0, have_u = 0;
        auto settle = [&](uint32_t &v, bool have, uint32_t start) {
          const uint32_t raw = v;
          v = kDenseSent;
          if (have) {
            v = raw - start;
            if (raw >= kDenseRemap) {
              const uint32_t sq = (raw - kDenseRemap) >> 10, pos = raw & (kDenseNear - 1u);
              v = pos >= start ? p.goff[seq_base + sq] + pos - start : kDenseSent;
            }
          }
        };
#pragma unroll 1
        for (int t = 0; t < R; ++t) {
          // (rolled, the arrays through selects: this path must stay small)
          uint32_t a_ = 0, b_ = 0;
#pragma unroll
          for (int q = 0; q < R; ++q) a_ = q == t ? val[q] : a_, b_ = q == t ? hv[q] : b_;
          uint32_t f_t = 0, st_t = 0;
#pragma unroll
          for (int q = 0; q < R; ++q) f_t = q == t ? f[q] : f_t, st_t = q == t ? st[q] : st_t;
          settle(a_, ln < f_t, st_t);
          settle(b_, long_lists && ln + (uint32_t)kWave < f_t, st_t);
          if (t < R - 1) {
            if (a_ < kDenseVLimit) mx = a_ > mx ? a_ : mx, have_u = 1;
            if (b_ < kDenseVLimit) mx = b_ > mx ? b_ : mx, have_u = 1;
          }
          if (kOptSent) a_ = a_ < kDenseVLimit ? a_ : sent_b;  // (a sentinel of the lane's own: no two dropped entries in one slot)
#pragma unroll
          for (int q = 0; q < R; ++q) val[q] = q == t ? a_ : val[q], hv[q] = q == t ? b_ : hv[q];
        }
        any_u = __builtin_amdgcn_ballot_w64(have_u != 0) != 0;
        max_u = wave_max_u32(mx);
        if (kOptSent && !kOptNoMask) {
#pragma unroll
          for (int t = 0; t < R; ++t) vm[t] = __builtin_amdgcn_ballot_w64(val[t] < kDenseVLimit);
        }
      } else {
        // every entry is real and lists ascend: the maximum of U is the largest last entry of runs 0..R-2
        if (kOptSent) {
          // a lane behind the list's end takes a sentinel of its own (sent_a - start: no two in one slot, fem_seed_join.hip.h
          // top) instead of the list's last entry again; which lanes hold entries stays behind as a scalar mask (kOptNoMask: it
          // does not — every such lane holds a value >= kDenseVLimit, which the flush of the flagged values tests once)
#pragma unroll
          for (int t = 0; t < R; ++t) {
            if (PADDED) {
              if (!kOptNoMask) vm[t] = __builtin_amdgcn_ballot_w64(ln < f[t]);  // (one v_cmp into a scalar pair; as scalar arithmetic on f it is six instructions)
              val[t] -= st[t];
            } else {
              const bool in = ln < f[t];
              if (!kOptNoMask) vm[t] = __builtin_amdgcn_ballot_w64(in);  // (the compare's own result: no instruction)
              val[t] = (in ? val[t] : sent_a) - st[t];
            }
          }
        } else {
#pragma unroll
          for (int t = 0; t < R; ++t) val[t] = PADDED ? val[t] - st[t] : ln < f[t] ? val[t] - st[t] : kDenseSent;  // (pads: sentinels already; the inserts test)
        }
        if (long_lists) {
#pragma unroll
          for (int t = 0; t < R; ++t) {
            if (PADDED && (!kOptLong || f[t] > (uint32_t)kWave))
              hv[t] -= st[t];  // (pads: "no entry" already)
            else
              hv[t] = ln + (uint32_t)kWave < f[t] ? hv[t] - st[t] : kDenseSent;
          }
#pragma unroll
          for (int t = 0; t < R - 1; ++t) {
            const uint32_t l_lo = (uint32_t)__builtin_amdgcn_readlane((int)val[t], (int)((f[t] - 1u) & 63u));
            const uint32_t l_hi = (uint32_t)__builtin_amdgcn_readlane((int)hv[t], (int)((f[t] - 65u) & 63u));
            const uint32_t lastv = f[t] > (uint32_t)kWave ? l_hi : l_lo;
            max_u = f[t] && lastv > max_u ? lastv : max_u;
          }
        } else {
#pragma unroll
          for (int t = 0; t < R - 1; ++t) {
            const uint32_t lastv = (uint32_t)__builtin_amdgcn_readlane((int)val[t], (int)((f[t] - 1u) & 63u));
            max_u = f[t] && lastv > max_u ? lastv : max_u;
          }
        }
      }
      if (keep_all) any_u = true, max_u = 0xFFFFFFFFu;
      if (any_u) {
        // the last run keeps values <= max(U) only (src/filter.c:85); everything dropped becomes a sentinel
        if (kOptSent) {
          const bool keep = val[R - 1] <= max_u;
          if (!kOptNoMask) vm[R - 1] &= __builtin_amdgcn_ballot_w64(keep);
          val[R - 1] = keep ? val[R - 1] : sent_b;
        } else {
          val[R - 1] = val[R - 1] <= max_u ? val[R - 1] : kDenseSent;
        }
        if (long_lists) hv[R - 1] = hv[R - 1] <= max_u ? hv[R - 1] : kDenseSent;
        // ---- insert, then flag (a neighbouring slot is present: the flagged values are compacted into the group's array).
        //      In batches of kBatch chunks: all of a batch's atomics back to back, its marks, later all of a batch's window
        //      reads before the first is used.  At R <= 6 a batch is the whole unit; above, one chunk — what a batch holds
        //      in registers (at R = 5 batches of 1, 2, 3 or 5 chunks run within 3 % of each other: the kernel is bound by
        //      instruction issue, not by the LDS round trips) (hit bits, window words) decides whether the kernel fits the 80 registers of six waves per SIMD,
        //      i.e. whether five of its blocks or four sit on a CU beside seed_select_kernel ----
        constexpr int kBatch = R > 6 ? FEM_JOIN_BATCH_HI : kPlain ? R : FEM_JOIN_BATCH_FULL < R ? FEM_JOIN_BATCH_FULL : R;
        // `exact`: the lanes without an entry are tested one by one (v < kDenseVLimit).  Otherwise `valid` says which lanes count
        // and a flagged lane WITHOUT an entry — always above the run's lanes with one: lists ascend, both ends of a run are
        // cut from the top — stores its sentinel at the place the next flagged value will take, or behind the last one,
        // where the exact filter reads it as "no value" (it lies above every coordinate).
        // kOptOnce, the forms without `exact`: a chunk only gathers — its flagged lanes' values into `fl`, their lanes into `acc` —
        // and the flagged values are compacted into the group's array by `flush`, when a lane is flagged a second time and once at
        // the unit's end.  A lane that holds no flagged value since the last flush has fl = 0xFFFFFFFF, a flagged lane without an
        // entry its sentinel: both >= kDenseVLimit, so the flush's one compare is the validity test (no sentinel is stored: behind
        // the values the array reads "no value" by join_read's fill).  Within a flush the values lie in lane order.
        uint32_t fl = 0xFFFFFFFFu;
        uint64_t acc = 0;
        auto flush = [&]() {
          const bool ok = fl < kDenseVLimit;
          const uint64_t m = __builtin_amdgcn_ballot_w64(ok);
          uint32_t pos = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, n_flag));
          pos = pos < kFlagCap ? pos : kFlagCap;
          if (ok) flg_g[pos] = fl;
          n_flag += (uint32_t)__popcll(m);
          fl = 0xFFFFFFFFu;
          acc = 0;
        };
        auto flag_chunk = [&](uint32_t v, uint32_t xw, uint64_t valid, bool exact) {
          if (FEM_JOIN_ABL & 1) {
            asm volatile("" ::"v"(xw), "v"(v));
            return;
          }
          if (kOptOnce && !exact) {
            const bool near_ = xw >= kNearTop;
            const uint64_t m = __builtin_amdgcn_ballot_w64(near_);
            if ((kOptNoMask ? m : m & valid) == 0) return;  // (wave-uniform)
            if ((m & acc) != 0) flush();
            fl = near_ ? v : fl;
            acc |= m;
            return;
          }
          bool near = xw >= kNearTop;
          if (exact) near = near && v < kDenseVLimit;
          const uint64_t m = exact ? __builtin_amdgcn_ballot_w64(near) : __builtin_amdgcn_ballot_w64(near) & valid;
          if (!exact && m == 0) return;  // (wave-uniform)
          uint32_t pos = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, n_flag));
          pos = pos < kFlagCap ? pos : kFlagCap;
          if (near) flg_g[pos] = v;
          n_flag += (uint32_t)__popcll(m);
        };
        auto insert_all = [&](uint32_t (&vals)[R], bool checked, bool second) {
#pragma unroll
          for (int t0 = 0; t0 < R; t0 += kBatch) {
            uint32_t hit[kBatch];
            LdsWord hw[kBatch];  // the word each insert addressed: the marks go there (kOptOwn; set wherever hit[q] can be non-zero)
#pragma unroll
            for (int q = 0; q < kBatch; ++q)
              if (t0 + q < R) {
                hit[q] = 0;
                if (second && kOptLong && f[t0 + q] <= (uint32_t)kWave) continue;
                hit[q] = checked ? insert(vals[t0 + q], hw[q]) : insert_plain(vals[t0 + q], hw[q]);
              }
            // a slot that took a second value (every true hit does): chunk by chunk, only where some lane saw one
#pragma unroll
            for (int q = 0; q < kBatch; ++q)
              if (t0 + q < R) {
                if (second && kOptLong && f[t0 + q] <= (uint32_t)kWave) continue;
                if (kOptHit) {
                  mark(vals[t0 + q], hit[q], hw[q]);
                } else if (__builtin_amdgcn_ballot_w64(hit[q] != 0u)) {
                  mark(vals[t0 + q], hit[q], hw[q]);
                }
              }
          }
        };
        auto flag_all = [&](uint32_t (&vals)[R], bool second, bool exact) {
#pragma unroll
          for (int t0 = 0; t0 < R; t0 += kBatch) {
            uint32_t x[kBatch];
#pragma unroll
            for (int q = 0; q < kBatch; ++q)
              if (t0 + q < R) {
                if (second && kOptLong && f[t0 + q] <= (uint32_t)kWave) continue;
                x[q] = window_top(vals[t0 + q]);
              }
#pragma unroll
            for (int q = 0; q < kBatch; ++q)
              if (t0 + q < R) {
                if (second && kOptLong && f[t0 + q] <= (uint32_t)kWave) continue;
                flag_chunk(vals[t0 + q], x[q], vm[t0 + q], exact);
              }
          }
          if (kOptOnce && !exact && acc != 0) flush();
        };
        if (FEM_JOIN_ABL & 64) {
#pragma unroll
          for (int t = 0; t < R; ++t) asm volatile("" ::"v"(val[t]), "v"(hv[t]));
        } else {
        insert_all(val, !kOptSent, false);
        if (long_lists) insert_all(hv, true, true);
        wave_sync_lds();
        if (!kOptSent || __builtin_expect(remap, 0)) flag_all(val, false, true); else flag_all(val, false, false);
        if (long_lists) flag_all(hv, true, true);  // (second chunks keep the compare against the sentinel: they are the exception)
        wave_sync_lds();
        }
        if (!(FEM_JOIN_ABL & 8)) {  // leave the bitmap clean: every lane clears its 16-byte pieces (the guard word sits behind them)
          uint4 *b4 = (uint4 *)bitmap;
#pragma unroll
          for (uint32_t k = 0; k < kWords / 4u / (uint32_t)kWave; ++k) b4[k * (uint32_t)kWave + ln] = make_uint4(0u, 0u, 0u, 0u);
        }
        wave_sync_lds();
        if (n_flag > kFlagCap) return false;
      }
