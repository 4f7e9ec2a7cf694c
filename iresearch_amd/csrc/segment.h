// segment.h — host side of a segment: open (staging, block directory, packed image, positions),
// the tables built on first use (posting-order norms, block-max data) and the segment-level entry
// points.  Included by irs_hip.hip (one translation unit).
#pragma once

struct irs_hip_segment {
  int device = 0;
  // the segment's name in the device's stream cache (an address comes back after a close)
  uint32_t uid = [] {
    static std::atomic<uint32_t> next{0};
    return ++next;
  }();
  DevSegment dev{};
  DevBuf d_doc, d_norms, d_terms, d_blk_off, d_blk_last, d_blk_bits, d_status;
  DevBuf d_blk_aoff, d_pk;     // packed-payload image (DevSegment::pk) and its offsets
  DevBuf d_blk_dir;            // BlkDir per block
  DevBuf d_blk_term;           // the row's term
  DevBuf d_tail_docs, d_tail_freqs;  // decoded vint tails, [num_terms][128]
  // positions (fields with POS): `.pos` bytes, per-term records, pos block directory,
  // positions in front of every doc block, decoded position tails
  DevBuf d_pos, d_pterms, d_pblk_off, d_pblk_bits, d_blk_pos, d_ptail;
  std::vector<DevPosTerm> pterms;
  std::vector<DevTerm> terms;  // host mirror incl. the fields the dir kernel filled
  uint64_t total_blocks = 0;
  uint64_t device_bytes = 0;
  uint32_t cus = 1;  // compute units of the device (persistent grid sizing)
  // Candidate slots per unit that batches on this segment turned out to need (recover_overflow):
  // scores that tie by the thousand at the threshold bin (TF-IDF without norms: every doc with
  // the same frequencies) cannot be cut by a bin threshold; later batches start from what the
  // earlier ones learned instead of overflowing and running twice each.  Decays never; bounded
  // by default_cand_cap's ceiling.
  std::atomic<uint32_t> cand_cap_hint{0};
  // block-max data (WAND), built on first use: the one thing that changes after open
  std::mutex wand_mutex;
  bool wand_ready = false;
  // the norm byte of every posting in posting order (k_posting_norms), built on the segment's
  // first joined batch; 1-byte Norm2 columns only
  DevBuf d_pnorm, d_tail_norms;
  bool pnorm_ready = false;
  DevBuf d_dead;                   // the DocumentMask as a bitmap (DevSegment::dead)
  uint64_t live_docs = 0;          // num_docs - deleted docs
  DevBuf d_blk_maxf, d_blk_minn;
  std::vector<uint64_t> skip_at;   // per term: absolute offset of its skip data (0: none)
  bool has_pos = false;
  uint64_t wand_from_index = 0;    // blocks whose (max freq, min norm) came from the index's wand data
  uint32_t wand_type = 0;          // IRS_HIP_WAND_* of the scorer that wrote the wand data
};

namespace {

// f(std::integral_constant<int, kSimd4 or kScalar>{}): the kernels' template argument of a block layout
template<typename F>
auto with_layout(int layout, F&& f) {
  return layout == kSimd4 ? f(std::integral_constant<int, kSimd4>{}) : f(std::integral_constant<int, kScalar>{});
}

bool device_usable(int device) {
  if (device < 0 || device >= rt::device_count()) return false;
  char arch[64] = {0};
  if (!rt::device_arch(device, arch, sizeof arch)) return false;
  // gfx950 only (the sim runtime of the CPU test tier reports "gfx950-sim")
  if (std::strncmp(arch, "gfx950", 6) != 0) return false;
  return rt::set_device(device);
}

// format_utils::check_header for `.doc` (format_utils.cpp:74-105,
// formats_10.cpp:325-326, 3356-3361); returns header length or 0.
size_t check_header(const uint8_t* f, uint64_t len, const char* name, int32_t* version) {
  const size_t nlen = std::strlen(name);
  if (len < 4 + 1 + nlen + 4 + 16) return 0;
  const uint32_t magic = (uint32_t(f[0]) << 24) | (uint32_t(f[1]) << 16) |
                         (uint32_t(f[2]) << 8) | f[3];
  if (magic != 0x3fd76c17u) return 0;
  if (f[4] != nlen || std::memcmp(f + 5, name, nlen) != 0) return 0;
  const uint8_t* v = f + 5 + nlen;
  *version = int32_t((uint32_t(v[0]) << 24) | (uint32_t(v[1]) << 16) |
                     (uint32_t(v[2]) << 8) | v[3]);
  return 5 + nlen + 4;
}
size_t check_doc_header(const uint8_t* f, uint64_t len, int32_t* version) {
  return check_header(f, len, "iresearch_10_postings_documents", version);
}
// `.pos`: formats_10.cpp:327-328, 3369-3381
size_t check_pos_header(const uint8_t* f, uint64_t len, int32_t* version) {
  return check_header(f, len, "iresearch_10_postings_positions", version);
}

// Packed-payload image: block sizes (left in blk_aoff by the directory kernel) ->
// exclusive prefix sum in place -> one copy pass.  Everything on the device.
// In-place exclusive prefix sum of n u32 values on the device; *total = their sum, which
// must fit 32 bits (the scanned values are offsets kept as u32).
int scan_exclusive(uint32_t* d_values, uint64_t n, uint64_t* total, bool may_wrap = false) {
  *total = 0;
  if (!n) return IRS_HIP_OK;
  const uint32_t parts = uint32_t((n + kScanChunk - 1) / kScanChunk);
  DevBuf totals;
  if (!totals.alloc((uint64_t(parts) + 1) * 8)) return IRS_HIP_ENOMEM;
  RT_LAUNCH(k_scan_totals, parts, kThreads, 0, nullptr, d_values, n, totals.as<uint64_t>());
  RT_LAUNCH(k_scan_parts, 1, 64, 0, nullptr, totals.as<uint64_t>(), parts);
  if (!rt::last_error_ok() || !rt::d2h(total, totals.as<uint64_t>() + parts, 8, nullptr) ||
      !rt::sync(nullptr))
    return IRS_HIP_EHIP;
  // (offsets kept as u32; sums that are only ever used as DIFFERENCES may wrap mod 2^32)
  if (*total > 0xFFFFFFFFull && !may_wrap) return IRS_HIP_EUNSUPPORTED;
  RT_LAUNCH(k_scan_apply, parts, kThreads, 0, nullptr, d_values, n, totals.as<uint64_t>());
  if (!rt::last_error_ok() || !rt::sync(nullptr)) return IRS_HIP_EHIP;
  return IRS_HIP_OK;
}

int build_packed_image(irs_hip_segment* s) {
  const uint64_t n = s->total_blocks;
  uint64_t total_units = 0;  // offsets are u32 units of 16 bytes (64 GB)
  if (const int rc = scan_exclusive(s->d_blk_aoff.as<uint32_t>(), n, &total_units)) return rc;
  if (n) {
    RT_LAUNCH(k_dir_aoff, uint32_t((n + kThreads - 1) / kThreads), kThreads, 0, nullptr,
              s->d_blk_aoff.as<uint32_t>(), n, s->d_blk_dir.as<BlkDir>());
    if (!rt::last_error_ok()) return IRS_HIP_EHIP;
  }
  const uint64_t bytes = total_units * 16;
  if (!s->d_pk.alloc(bytes + kPadBytes)) return IRS_HIP_ENOMEM;
  if (!rt::dmemset(s->d_pk.as<uint8_t>() + bytes, 0, kPadBytes, nullptr)) return IRS_HIP_EHIP;
  s->dev.pk = s->d_pk.as<uint8_t>();
  if (total_units && n) {
    RT_LAUNCH(k_pack_payloads, row_grid(n, s->cus), kThreads, 0, nullptr, s->dev, n,
              s->d_pk.as<uint8_t>());
    if (!rt::last_error_ok() || !rt::sync(nullptr)) return IRS_HIP_EHIP;
  }
  return IRS_HIP_OK;
}

template<int LAYOUT>
int build_directory(irs_hip_segment* s) {
  const uint32_t grid = s->dev.num_terms;   // a workgroup per term
  if (!rt::dmemset(s->d_status.p, 0, 4, nullptr)) return IRS_HIP_EHIP;
  if (grid) {
    RT_LAUNCH((k_build_directory<LAYOUT>), grid, kChainThreads, 0, nullptr, s->dev,
              s->d_terms.as<DevTerm>(), s->d_blk_off.as<uint32_t>(),
              s->d_blk_last.as<uint32_t>(), s->d_blk_bits.as<uint16_t>(),
              s->d_blk_aoff.as<uint32_t>(), s->d_blk_dir.as<BlkDir>(),
              s->d_blk_term.as<uint32_t>(),
              s->d_tail_docs.as<uint32_t>(), s->d_tail_freqs.as<uint32_t>(),
              s->d_status.as<uint32_t>());
  }
  if (!rt::last_error_ok()) return IRS_HIP_EHIP;
  uint32_t status = 0;
  if (!rt::d2h(&status, s->d_status.p, 4, nullptr) ||
      !rt::d2h(s->terms.data(), s->d_terms.p, s->terms.size() * sizeof(DevTerm), nullptr) ||
      !rt::sync(nullptr))
    return IRS_HIP_EHIP;
  if (status & kStatusCorrupt) return IRS_HIP_ECORRUPT;
  for (const DevTerm& t : s->terms) {
    if (t.docs_count && (t.last_doc > s->dev.num_docs || t.last_doc < kDocMin))
      return IRS_HIP_ECORRUPT;
  }
  return build_packed_image(s);
}

// Positions: frequency sums per doc block -> exclusive scan (blk_pos), then the pos block
// directory and the decoded position tails.  `pos_end` = term_meta::pos_end per term.
template<int LAYOUT>
int build_positions(irs_hip_segment* s, const std::vector<uint64_t>& pos_end) {
  const uint64_t n = s->total_blocks;
  if (!rt::dmemset(s->d_blk_pos.p, 0, s->d_blk_pos.n, nullptr)) return IRS_HIP_EHIP;
  if (n && s->dev.num_terms) {
    RT_LAUNCH((k_freq_sums<LAYOUT>), row_grid(n, s->cus), kThreads, 0, nullptr, s->dev,
              n, s->d_blk_pos.as<uint32_t>());
    if (!rt::last_error_ok() || !rt::sync(nullptr)) return IRS_HIP_EHIP;
  }
  uint64_t total = 0;
  // (position numbers are per term: differences of blk_pos, every term's total < 2^32)
  if (const int rc = scan_exclusive(s->d_blk_pos.as<uint32_t>(), n, &total, true)) return rc;
  const uint32_t total32 = uint32_t(total);  // sentinel row: everything in front of "row n"
  if (!rt::h2d(s->d_blk_pos.as<uint32_t>() + n, &total32, 4, nullptr)) return IRS_HIP_EHIP;
  DevBuf d_pos_end;
  if (!d_pos_end.alloc(std::max<size_t>(1, pos_end.size()) * 8)) return IRS_HIP_ENOMEM;
  if (!rt::h2d(d_pos_end.p, pos_end.data(), pos_end.size() * 8, nullptr) ||
      !rt::dmemset(s->d_status.p, 0, 4, nullptr))
    return IRS_HIP_EHIP;
  const uint32_t grid = (s->dev.num_terms + kWaves - 1) / kWaves;
  if (grid) {
    // a term_meta::freq that disagrees with the decoded frequencies would send the position
    // kernels past their buffers: refuse the segment (IRS_HIP_ECORRUPT)
    RT_LAUNCH(k_check_freq_totals, (s->dev.num_terms + kThreads - 1) / kThreads, kThreads, 0,
              nullptr, s->dev, s->d_pterms.as<DevPosTerm>(), s->d_status.as<uint32_t>());
    RT_LAUNCH(k_pos_directory, s->dev.num_terms, kChainThreads, 0, nullptr, s->dev, s->d_pterms.as<DevPosTerm>(),
              s->d_pblk_off.as<uint32_t>(), s->d_pblk_bits.as<uint8_t>(),
              s->d_ptail.as<uint32_t>(), d_pos_end.as<uint64_t>(), s->d_status.as<uint32_t>());
  }
  uint32_t status = 0;
  if (!rt::last_error_ok() || !rt::d2h(&status, s->d_status.p, 4, nullptr) ||
      !rt::d2h(s->pterms.data(), s->d_pterms.p, s->pterms.size() * sizeof(DevPosTerm), nullptr) ||
      !rt::sync(nullptr))
    return IRS_HIP_EHIP;
  return (status & kStatusCorrupt) ? IRS_HIP_ECORRUPT : IRS_HIP_OK;
}

// Block-max data of a segment (conj.h k_block_max), built once, on first use.
static bool launch_block_max(irs_hip_segment* s) {
  const uint64_t rows = s->total_blocks;
  with_layout(s->dev.layout, [&](auto L) {
    RT_LAUNCH((k_block_max<decltype(L)::value>), row_grid(rows, s->cus), kThreads, 0, nullptr, s->dev,
              rows, s->d_blk_maxf.as<uint32_t>(), s->d_blk_minn.as<uint32_t>());
  });
  return rt::last_error_ok() && rt::sync(nullptr);
}

int prepare_posting_norms(irs_hip_segment* s) {
  std::lock_guard<std::mutex> lock(s->wand_mutex);
  if (s->pnorm_ready) return IRS_HIP_OK;
  const DevSegment& d = s->dev;
  if (d.norms && d.norm_width == 1u && !d.norm_legacy) {
    const uint64_t rows = s->total_blocks, tails = s->d_tail_docs.n / 4;
    if (!s->d_pnorm.alloc((rows + 1) * kBlock) || !s->d_tail_norms.alloc(tails + 1))
      return IRS_HIP_ENOMEM;
    if (rows && d.num_terms) {
      with_layout(d.layout, [&](auto L) {
        RT_LAUNCH((k_posting_norms<decltype(L)::value>), row_grid(rows, s->cus), kThreads, 0, nullptr, d, rows,
                  s->d_pnorm.as<uint8_t>());
      });
    }
    if (tails) {
      RT_LAUNCH(k_tail_norms, uint32_t((tails + kThreads - 1) / kThreads), kThreads, 0, nullptr, d,
                tails, s->d_tail_norms.as<uint8_t>());
    }
    if (!rt::last_error_ok() || !rt::sync(nullptr)) return IRS_HIP_EHIP;
    s->device_bytes += s->d_pnorm.n + s->d_tail_norms.n;
    s->dev.pnorm = s->d_pnorm.as<uint8_t>();
    s->dev.tail_norms = s->d_tail_norms.as<uint8_t>();
  }
  s->pnorm_ready = true;
  return IRS_HIP_OK;
}

int prepare_blockmax(irs_hip_segment* s) {
  std::lock_guard<std::mutex> lock(s->wand_mutex);
  if (s->wand_ready) return IRS_HIP_OK;
  const uint64_t n = s->total_blocks;
  if (!s->d_blk_maxf.alloc((n + 1) * 4) || !s->d_blk_minn.alloc((n + 1) * 4)) return IRS_HIP_ENOMEM;
  if (n && s->dev.num_terms) {
    // derived from the postings: every block of every index gets a pair
    if (!launch_block_max(s)) return IRS_HIP_EHIP;
    // a field indexed with scorers carries the pairs itself (skip level 0): those are used —
    // when they bound EVERY score function: a MaxFreq or MinNorm payload.  A DivNorm payload
    // is the (freq, norm) of the doc with the largest ratio, no bound for BM25 or a MaxFreq
    // scorer (the reference refuses the combination: Scorer::compatible, scorer.cpp:46-49)
    if (!s->skip_at.empty() &&
        (s->wand_type == IRS_HIP_WAND_MAX_FREQ || s->wand_type == IRS_HIP_WAND_MIN_NORM)) {
      DevBuf d_at, d_taken;
      if (!d_at.alloc(s->skip_at.size() * 8) || !d_taken.alloc(8)) return IRS_HIP_ENOMEM;
      uint32_t status = 0;
      unsigned long long taken = 0;
      if (!rt::h2d(d_at.p, s->skip_at.data(), s->skip_at.size() * 8, nullptr) ||
          !rt::dmemset(d_taken.p, 0, 8, nullptr) || !rt::dmemset(s->d_status.p, 0, 4, nullptr))
        return IRS_HIP_EHIP;
      RT_LAUNCH(k_wand_skip0, s->dev.num_terms, kChainThreads, 0, nullptr,
                s->dev, d_at.as<uint64_t>(), s->has_pos ? 1u : 0u, s->d_blk_maxf.as<uint32_t>(),
                s->d_blk_minn.as<uint32_t>(), d_taken.as<unsigned long long>(),
                s->d_status.as<uint32_t>());
      if (!rt::last_error_ok() || !rt::d2h(&status, s->d_status.p, 4, nullptr) ||
          !rt::d2h(&taken, d_taken.p, 8, nullptr) || !rt::sync(nullptr))
        return IRS_HIP_EHIP;
      if (status & kStatusCorrupt) return IRS_HIP_ECORRUPT;
      if (status & kStatusWandFraming) {
        // entries that do not line up with the block directory (e.g. a field with positions
        // opened without its `.pos`): nothing of the walk is trusted, the derived pairs stand
        if (!launch_block_max(s)) return IRS_HIP_EHIP;
        taken = 0;
      }
      s->wand_from_index = taken;
    }
  }
  s->dev.blk_maxf = s->d_blk_maxf.as<uint32_t>();
  s->dev.blk_minn = s->d_blk_minn.as<uint32_t>();
  s->device_bytes += s->d_blk_maxf.n + s->d_blk_minn.n;
  s->wand_ready = true;
  return IRS_HIP_OK;
}

static int segment_open_impl(const irs_hip_segment_desc* d, irs_hip_segment** out) {
  if (!d || !out) return IRS_HIP_EINVAL;
  *out = nullptr;
  if (!d->doc_file || !d->num_docs || d->num_docs > 0x7FFF0000u ||
      (d->layout != IRS_HIP_LAYOUT_SCALAR && d->layout != IRS_HIP_LAYOUT_SIMD4) ||
      (d->num_terms && !d->terms) || d->wand_count > 16 || d->wand_type > IRS_HIP_WAND_MIN_NORM ||
      (d->doc_mask_count && !d->doc_mask))
    return IRS_HIP_EINVAL;
  if (d->norm_kind != IRS_HIP_NORM2 && d->norm_kind != IRS_HIP_NORM_LEGACY) return IRS_HIP_EINVAL;
  if (d->norms) {
    if (d->norm_width != 1 && d->norm_width != 2 && d->norm_width != 4) return IRS_HIP_EINVAL;
    if (d->norm_kind == IRS_HIP_NORM_LEGACY && d->norm_width != 4) return IRS_HIP_EINVAL;
    // dense column covering every doc (columnstore2.cpp:650-789); sparse columns
    // are not on the benchmark path
    if (d->norm_min_doc != kDocMin || d->norm_count < d->num_docs) return IRS_HIP_EUNSUPPORTED;
  }
  int32_t version = -1;
  const size_t hdr = check_doc_header(d->doc_file, d->doc_file_len, &version);
  if (!hdr) return IRS_HIP_ECORRUPT;
  if (d->doc_file_len >= 0xFFFFFF00ull) return IRS_HIP_EUNSUPPORTED;  // block offsets are u32
  // PostingsFormat: odd versions are the SSE (simd4) layouts (formats_10.cpp:283-313)
  if (version < 0 || version > 5) return IRS_HIP_ECORRUPT;
  if ((version & 1) != (d->layout == IRS_HIP_LAYOUT_SIMD4 ? 1 : 0)) return IRS_HIP_EINVAL;
  size_t pos_hdr = 0;
  if (d->pos_file) {
    // positions need frequencies (IndexFeatures::POS implies FREQ)
    int32_t pos_version = -1;
    pos_hdr = check_pos_header(d->pos_file, d->pos_file_len, &pos_version);
    if (!pos_hdr) return IRS_HIP_ECORRUPT;
    if (pos_version != version) return IRS_HIP_ECORRUPT;
    if (!d->has_freq) return IRS_HIP_EINVAL;
    if (d->pos_features & ~(IRS_HIP_POS_OFFSETS | IRS_HIP_POS_PAYLOADS)) return IRS_HIP_EINVAL;
    if (d->pos_features) return IRS_HIP_EUNSUPPORTED;  // the `.pos` tail interleaves them
  }
  if (!device_usable(d->device)) return IRS_HIP_EHIP;

  irs_hip_segment* s = new (std::nothrow) irs_hip_segment;
  if (!s) return IRS_HIP_ENOMEM;
  s->device = d->device;
  s->cus = std::max(1, rt::device_cus(d->device));
  int rc = IRS_HIP_OK;
  do {
    try {
      s->terms.resize(d->num_terms);
    } catch (...) {
      rc = IRS_HIP_ENOMEM;
      break;
    }
    uint64_t blocks = 0, tail_rows = 0;
    for (uint32_t i = 0; i < d->num_terms && rc == IRS_HIP_OK; ++i) {
      const irs_hip_term_meta& m = d->terms[i];
      DevTerm t{};
      t.docs_count = m.docs_count;
      t.tail_row = uint32_t(tail_rows);
      tail_rows += m.docs_count == 1 ? 1u : m.docs_count % kBlock;
      if (tail_rows > 0xFFFFFF00ull) rc = IRS_HIP_EUNSUPPORTED;
      if (m.docs_count == 1) {
        t.single_doc = kDocMin + uint32_t(m.e_skip_start);  // formats_10.cpp:1887
        t.single_freq = m.freq;
        t.doc_start = 0;
      } else if (m.docs_count > 1) {
        if (m.doc_start < hdr || m.doc_start >= d->doc_file_len) rc = IRS_HIP_ECORRUPT;
        t.doc_start = m.doc_start;
        t.nblk = m.docs_count / kBlock;
        t.tail_n = m.docs_count % kBlock;
        t.dir_off = blocks;
        blocks += t.nblk;
        // block offsets are kept as u32 relative to doc_start
        if (m.docs_count > kBlock && m.e_skip_start > 0xFFFFFFFFull) rc = IRS_HIP_EUNSUPPORTED;
        if (m.docs_count > kBlock && d->wand_count) {
          if (s->skip_at.empty()) s->skip_at.assign(d->num_terms, 0);
          s->skip_at[i] = m.doc_start + m.e_skip_start;
          if (s->skip_at[i] >= d->doc_file_len) rc = IRS_HIP_ECORRUPT;
        }
      }
      s->terms[i] = t;
    }
    if (rc != IRS_HIP_OK) break;
    s->total_blocks = blocks;
    s->has_pos = d->pos_file != nullptr;
    s->wand_type = d->wand_type;
    const uint64_t norm_bytes = d->norms ? uint64_t(d->norm_width) * d->norm_count : 0;
    if (!s->d_doc.alloc(d->doc_file_len + kPadBytes) ||
        (d->norms && !s->d_norms.alloc(norm_bytes + kPadBytes)) ||
        !s->d_terms.alloc(std::max<size_t>(1, s->terms.size()) * sizeof(DevTerm)) ||
        !s->d_blk_off.alloc((blocks + 1) * 4) || !s->d_blk_last.alloc((blocks + 1) * 4) ||
        !s->d_blk_bits.alloc((blocks + 1) * 2) || !s->d_blk_aoff.alloc((blocks + 1) * 4) ||
        !s->d_blk_dir.alloc((blocks + 1) * sizeof(BlkDir)) ||
        !s->d_blk_term.alloc((blocks + 1) * 4) ||
        !s->d_tail_docs.alloc((tail_rows + 1) * 4) || !s->d_tail_freqs.alloc((tail_rows + 1) * 4) ||
        !s->d_status.alloc(4)) {
      rc = IRS_HIP_ENOMEM;
      break;
    }
    bool okc = rt::h2d(s->d_doc.p, d->doc_file, d->doc_file_len, nullptr) &&
               rt::dmemset(s->d_doc.as<uint8_t>() + d->doc_file_len, 0, kPadBytes, nullptr) &&
               rt::h2d(s->d_terms.p, s->terms.data(), s->terms.size() * sizeof(DevTerm), nullptr);
    if (d->norms) {
      okc = okc && rt::h2d(s->d_norms.p, d->norms, norm_bytes, nullptr) &&
            rt::dmemset(s->d_norms.as<uint8_t>() + norm_bytes, 0, kPadBytes, nullptr);
    }
    if (!okc || !rt::sync(nullptr)) {
      rc = IRS_HIP_EHIP;
      break;
    }
    DevSegment& v = s->dev;
    v.doc = s->d_doc.as<uint8_t>();
    v.doc_len = d->doc_file_len;
    v.norms = d->norms ? s->d_norms.as<uint8_t>() : nullptr;
    v.norm_width = d->norms ? d->norm_width : 0;
    v.norm_min_doc = d->norms ? d->norm_min_doc : kDocMin;
    v.norm_count = d->norms ? d->norm_count : 0;
    v.norm_legacy = (d->norms && d->norm_kind == IRS_HIP_NORM_LEGACY) ? 1u : 0u;
    v.terms = s->d_terms.as<DevTerm>();
    v.num_terms = d->num_terms;
    v.num_docs = d->num_docs;
    v.blk_off = s->d_blk_off.as<uint32_t>();
    v.blk_last = s->d_blk_last.as<uint32_t>();
    v.blk_bits = s->d_blk_bits.as<uint16_t>();
    v.blk_aoff = s->d_blk_aoff.as<uint32_t>();
    v.blk_dir = s->d_blk_dir.as<BlkDir>();
    v.blk_term = s->d_blk_term.as<uint32_t>();
    v.tail_docs = s->d_tail_docs.as<uint32_t>();
    v.tail_freqs = s->d_tail_freqs.as<uint32_t>();
    v.pk = nullptr;  // set by build_packed_image
    v.has_freq = d->has_freq ? 1 : 0;
    v.layout = d->layout;
    v.wand_count = d->wand_count;
    s->live_docs = d->num_docs;
    if (d->doc_mask_count) {
      // DocumentMask -> bitmap, bit (doc - kDocMin) (dead_words, excl.h)
      const uint64_t words = dead_words(d->num_docs);
      std::vector<uint32_t> bits;
      try {
        bits.assign(words, 0u);
      } catch (...) {
        rc = IRS_HIP_ENOMEM;
        break;
      }
      uint64_t gone = 0;
      for (uint64_t i = 0; i < d->doc_mask_count; ++i) {
        const uint32_t doc = d->doc_mask[i];
        if (doc < kDocMin || doc > d->num_docs) continue;
        const uint32_t j = doc - kDocMin;
        gone += (bits[j >> 5] >> (j & 31u)) & 1u ? 0u : 1u;
        bits[j >> 5] |= 1u << (j & 31u);
      }
      if (gone) {
        if (!s->d_dead.alloc(words * 4)) {
          rc = IRS_HIP_ENOMEM;
          break;
        }
        if (!rt::h2d(s->d_dead.p, bits.data(), words * 4, nullptr) || !rt::sync(nullptr)) {
          rc = IRS_HIP_EHIP;
          break;
        }
        v.dead = s->d_dead.as<uint32_t>();
        s->live_docs = d->num_docs - gone;
      }
    }
    rc = d->layout == IRS_HIP_LAYOUT_SIMD4 ? build_directory<kSimd4>(s)
                                           : build_directory<kScalar>(s);
    if (rc == IRS_HIP_OK && d->pos_file) {
      std::vector<uint64_t> pos_end;
      uint64_t rows = 0, ptail_rows = 0;
      try {
        s->pterms.resize(d->num_terms);
        pos_end.resize(d->num_terms);
      } catch (...) {
        rc = IRS_HIP_ENOMEM;
        break;
      }
      for (uint32_t i = 0; i < d->num_terms && rc == IRS_HIP_OK; ++i) {
        const irs_hip_term_meta& m = d->terms[i];
        DevPosTerm pt{};
        if (m.docs_count) {
          if (m.freq < m.docs_count || m.pos_start < pos_hdr || m.pos_start > d->pos_file_len)
            rc = IRS_HIP_ECORRUPT;
          pt.pos_start = m.pos_start;
          pt.total = m.freq;
          pt.nfull = m.freq / kBlock;
          pt.tail_n = m.freq % kBlock;
          pt.row = rows;
          rows += pt.nfull;
          pt.tail_row = uint32_t(ptail_rows);
          ptail_rows += pt.tail_n;
          if (ptail_rows > 0xFFFFFF00ull) rc = IRS_HIP_EUNSUPPORTED;
        }
        s->pterms[i] = pt;
        pos_end[i] = m.pos_end;
      }
      if (rc != IRS_HIP_OK) break;
      if (!s->d_pos.alloc(d->pos_file_len + kPadBytes) ||
          !s->d_pterms.alloc(std::max<size_t>(1, s->pterms.size()) * sizeof(DevPosTerm)) ||
          !s->d_pblk_off.alloc((rows + 1) * 4) || !s->d_pblk_bits.alloc(rows + 1) ||
          !s->d_blk_pos.alloc((blocks + 1) * 4) ||
          !s->d_ptail.alloc((ptail_rows + 1) * 4)) {
        rc = IRS_HIP_ENOMEM;
        break;
      }
      if (!rt::h2d(s->d_pos.p, d->pos_file, d->pos_file_len, nullptr) ||
          !rt::dmemset(s->d_pos.as<uint8_t>() + d->pos_file_len, 0, kPadBytes, nullptr) ||
          !rt::h2d(s->d_pterms.p, s->pterms.data(), s->pterms.size() * sizeof(DevPosTerm),
                   nullptr) ||
          !rt::sync(nullptr)) {
        rc = IRS_HIP_EHIP;
        break;
      }
      v.pos = s->d_pos.as<uint8_t>();
      v.pos_len = d->pos_file_len;
      v.pterms = s->d_pterms.as<DevPosTerm>();
      v.pblk_off = s->d_pblk_off.as<uint32_t>();
      v.pblk_bits = s->d_pblk_bits.as<uint8_t>();
      v.blk_pos = s->d_blk_pos.as<uint32_t>();
      v.ptail = s->d_ptail.as<uint32_t>();
      // PostingsFormat < POSITIONS_ZEROBASED (formats_10.cpp:283-304): one-based storage
      v.pos_base = version < 2 ? 1u : 0u;
      rc = d->layout == IRS_HIP_LAYOUT_SIMD4 ? build_positions<kSimd4>(s, pos_end)
                                             : build_positions<kScalar>(s, pos_end);
    }
    s->device_bytes = s->d_doc.n + s->d_norms.n + s->d_terms.n + s->d_blk_off.n +
                      s->d_blk_last.n + s->d_blk_bits.n + s->d_blk_aoff.n + s->d_blk_dir.n + s->d_blk_term.n + s->d_pk.n +
                      s->d_tail_docs.n + s->d_tail_freqs.n + s->d_pos.n + s->d_pterms.n +
                      s->d_pblk_off.n + s->d_pblk_bits.n + s->d_blk_pos.n + s->d_ptail.n + s->d_dead.n;
  } while (false);
  if (rc != IRS_HIP_OK) {
    delete s;
    return rc;
  }
  *out = s;
  return IRS_HIP_OK;
}

static int decode_term_impl(irs_hip_segment* seg, uint32_t term, uint32_t* docs, uint32_t* freqs,
                        uint32_t cap, uint32_t* count) {
  if (!seg || !docs || !count || term >= seg->dev.num_terms) return IRS_HIP_EINVAL;
  if (freqs && !seg->dev.has_freq) return IRS_HIP_EINVAL;
  if (!rt::set_device(seg->device)) return IRS_HIP_EHIP;
  const DevTerm& t = seg->terms[term];
  *count = t.docs_count;
  if (t.docs_count == 0) return IRS_HIP_OK;
  if (cap < t.docs_count) return IRS_HIP_EINVAL;
  DevBuf dd, df;
  const size_t bytes = size_t(t.docs_count) * 4;
  if (!dd.alloc(bytes) || (freqs && !df.alloc(bytes))) return IRS_HIP_ENOMEM;
  const uint32_t items = t.nblk + 1;
  const uint32_t grid = (items + kWaves - 1) / kWaves;
  with_layout(seg->dev.layout, [&](auto L) {
    RT_LAUNCH((k_decode_term<decltype(L)::value>), grid, kThreads, 0, nullptr, seg->dev, term,
              dd.as<uint32_t>(), freqs ? df.as<uint32_t>() : nullptr);
  });
  if (!rt::last_error_ok() || !rt::d2h(docs, dd.p, bytes, nullptr) ||
      (freqs && !rt::d2h(freqs, df.p, bytes, nullptr)) || !rt::sync(nullptr))
    return IRS_HIP_EHIP;
  return IRS_HIP_OK;
}

static int decode_positions_impl(irs_hip_segment* seg, uint32_t term, uint32_t* positions,
                             uint64_t cap, uint64_t* count) {
  if (!seg || !positions || !count || term >= seg->dev.num_terms) return IRS_HIP_EINVAL;
  if (!seg->dev.pos) return IRS_HIP_EINVAL;  // the segment was opened without `.pos`
  if (!rt::set_device(seg->device)) return IRS_HIP_EHIP;
  const DevTerm& t = seg->terms[term];
  const uint64_t total = seg->pterms[term].total;
  *count = total;
  if (t.docs_count == 0 || total == 0) return IRS_HIP_OK;
  if (cap < total) return IRS_HIP_EINVAL;
  DevBuf dp;
  if (!dp.alloc(size_t(total) * 4)) return IRS_HIP_ENOMEM;
  const uint32_t items = t.nblk + 1;
  const uint32_t grid = (items + kWaves - 1) / kWaves;
  with_layout(seg->dev.layout, [&](auto L) {
    RT_LAUNCH((k_decode_positions<decltype(L)::value>), grid, kThreads, 0, nullptr, seg->dev, term,
              dp.as<uint32_t>());
  });
  if (!rt::last_error_ok() || !rt::d2h(positions, dp.p, size_t(total) * 4, nullptr) ||
      !rt::sync(nullptr))
    return IRS_HIP_EHIP;
  return IRS_HIP_OK;
}

static int bit_union_impl(irs_hip_segment* seg, const uint32_t* terms, uint32_t n_terms,
                      uint64_t* set, uint64_t n_words, uint64_t* count) {
  if (!seg || (!terms && n_terms) || !set || !n_words) return IRS_HIP_EINVAL;
  if (!rt::set_device(seg->device)) return IRS_HIP_EHIP;
  uint64_t total = 0;
  for (uint32_t i = 0; i < n_terms; ++i) {
    if (terms[i] == IRS_HIP_NO_TERM) continue;
    if (terms[i] >= seg->dev.num_terms) return IRS_HIP_EINVAL;
    total += seg->terms[terms[i]].docs_count;  // formats_10.cpp:3796, 3802
  }
  if (count) *count = total;
  if (!n_terms) return IRS_HIP_OK;
  // work list: up to kUnionBlocks blocks of one term per workgroup (+ its tail)
  std::vector<UnionWg> wgs;
  try {
    for (uint32_t i = 0; i < n_terms; ++i) {
      if (terms[i] == IRS_HIP_NO_TERM) continue;
      const DevTerm& t = seg->terms[terms[i]];
      if (t.docs_count == 0) continue;
      uint32_t b = 0;
      do {
        wgs.push_back(UnionWg{terms[i], b, 0u, 0u});
        b += kUnionBlocks;
      } while (b < t.nblk);
    }
  } catch (...) {
    return IRS_HIP_ENOMEM;
  }
  if (wgs.empty()) return IRS_HIP_OK;
  if (wgs.size() > 0x7FFFFFFFull) return IRS_HIP_EUNSUPPORTED;
  DevBuf d_wgs, d_set;
  const size_t set_bytes = size_t(n_words) * 8;
  if (!d_wgs.alloc(wgs.size() * sizeof(UnionWg)) || !d_set.alloc(set_bytes)) return IRS_HIP_ENOMEM;
  // (bits already set by the caller are kept: the set goes up first.  Round 6 tried to leave the
  // upload out when the caller's set is empty — a scan of it + a device memset — and to stage the
  // result through page-locked memory of the pool: 0.39 and 0.54 ms per call against 0.245; the
  // runtime's own staging of pageable copies is the fastest of the three at 1.25 MB.)
  if (!rt::h2d(d_wgs.p, wgs.data(), wgs.size() * sizeof(UnionWg), nullptr) ||
      !rt::h2d(d_set.p, set, set_bytes, nullptr))
    return IRS_HIP_EHIP;
  const uint64_t n_bits = n_words * 64;
  with_layout(seg->dev.layout, [&](auto L) {
    RT_LAUNCH((k_bit_union<decltype(L)::value>), uint32_t(wgs.size()), kThreads, 0, nullptr, seg->dev,
              d_wgs.as<UnionWg>(), d_set.as<uint32_t>(), n_bits);
  });
  if (!rt::last_error_ok() || !rt::d2h(set, d_set.p, set_bytes, nullptr) || !rt::sync(nullptr))
    return IRS_HIP_EHIP;
  return IRS_HIP_OK;
}

// Several unions at once, only their populations coming back: the bitsets stay on the device
// (one per set of a pass; passes of at most ~1 GB of them).
static int bit_union_counts_impl(irs_hip_segment* seg, const uint32_t* terms, const uint32_t* offsets,
                                 uint32_t n_sets, uint64_t* counts) {
  if (!seg || !offsets || !counts || (!terms && n_sets && offsets[n_sets] != offsets[0])) return IRS_HIP_EINVAL;
  if (!rt::set_device(seg->device)) return IRS_HIP_EHIP;
  for (uint32_t i = 0; i < n_sets; ++i) {
    if (offsets[i + 1] < offsets[i]) return IRS_HIP_EINVAL;
    counts[i] = 0;
  }
  if (!n_sets) return IRS_HIP_OK;
  for (uint32_t i = offsets[0]; i < offsets[n_sets]; ++i)
    if (terms[i] != IRS_HIP_NO_TERM && terms[i] >= seg->dev.num_terms) return IRS_HIP_EINVAL;
  const uint64_t n_words = (uint64_t(seg->dev.num_docs) + 64) / 64;   // bit index = doc id
  const uint64_t words32 = n_words * 2, n_bits = n_words * 64;
  const uint32_t per_pass = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(n_sets, (1ull << 30) / (n_words * 8))));
  DevBuf d_sets, d_wgs, d_counts;
  if (!d_sets.alloc(uint64_t(per_pass) * n_words * 8) || !d_counts.alloc(uint64_t(per_pass) * 8)) return IRS_HIP_ENOMEM;
  std::vector<UnionWg> wgs;
  std::vector<unsigned long long> got(per_pass);
  for (uint32_t s0 = 0; s0 < n_sets; s0 += per_pass) {
    const uint32_t ns = std::min(per_pass, n_sets - s0);
    wgs.clear();
    for (uint32_t s = 0; s < ns; ++s) {
      for (uint32_t i = offsets[s0 + s]; i < offsets[s0 + s + 1]; ++i) {
        if (terms[i] == IRS_HIP_NO_TERM) continue;
        const DevTerm& t = seg->terms[terms[i]];
        if (t.docs_count == 0) continue;
        uint32_t b = 0;
        do {
          wgs.push_back(UnionWg{terms[i], b, s, 0u});
          b += kUnionBlocks;
        } while (b < t.nblk);
      }
    }
    if (wgs.size() > 0x7FFFFFFFull) return IRS_HIP_EUNSUPPORTED;
    if (!rt::dmemset(d_sets.p, 0, uint64_t(ns) * n_words * 8, nullptr)) return IRS_HIP_EHIP;
    if (!wgs.empty()) {
      if (!d_wgs.alloc(wgs.size() * sizeof(UnionWg))) return IRS_HIP_ENOMEM;
      if (!rt::h2d(d_wgs.p, wgs.data(), wgs.size() * sizeof(UnionWg), nullptr)) return IRS_HIP_EHIP;
      with_layout(seg->dev.layout, [&](auto L) {
        RT_LAUNCH((k_bit_union<decltype(L)::value>), uint32_t(wgs.size()), kThreads, 0, nullptr, seg->dev,
                  d_wgs.as<UnionWg>(), d_sets.as<uint32_t>(), n_bits);
      });
    }
    RT_LAUNCH(k_union_counts, ns, kThreads, 0, nullptr, d_sets.as<uint32_t>(), words32,
              d_counts.as<unsigned long long>());
    if (!rt::last_error_ok() || !rt::d2h(got.data(), d_counts.p, uint64_t(ns) * 8, nullptr) || !rt::sync(nullptr))
      return IRS_HIP_EHIP;
    for (uint32_t s = 0; s < ns; ++s) counts[s0 + s] = got[s];
  }
  return IRS_HIP_OK;
}

static int term_directory_impl(irs_hip_segment* seg, uint32_t term, uint32_t* last_docs,
                           uint64_t* offsets, uint32_t cap, uint32_t* count) {
  if (!seg || !count || term >= seg->dev.num_terms) return IRS_HIP_EINVAL;
  if (!rt::set_device(seg->device)) return IRS_HIP_EHIP;
  const DevTerm& t = seg->terms[term];
  *count = t.nblk;
  if (!t.nblk) return IRS_HIP_OK;
  if (cap < t.nblk || !last_docs || !offsets) return IRS_HIP_EINVAL;
  std::vector<uint32_t> rel(t.nblk);
  if (!rt::d2h(last_docs, seg->d_blk_last.as<uint32_t>() + t.dir_off, size_t(t.nblk) * 4,
               nullptr) ||
      !rt::d2h(rel.data(), seg->d_blk_off.as<uint32_t>() + t.dir_off, size_t(t.nblk) * 4,
               nullptr) ||
      !rt::sync(nullptr))
    return IRS_HIP_EHIP;
  for (uint32_t i = 0; i < t.nblk; ++i) offsets[i] = t.doc_start + rel[i];
  return IRS_HIP_OK;
}

static int term_blockmax_impl(irs_hip_segment* seg, uint32_t term, uint32_t* max_freqs,
                              uint32_t* min_norms, uint32_t cap, uint32_t* count) {
  if (!seg || !count || term >= seg->dev.num_terms) return IRS_HIP_EINVAL;
  if (!rt::set_device(seg->device)) return IRS_HIP_EHIP;
  const DevTerm& t = seg->terms[term];
  *count = t.nblk;
  if (!t.nblk) return IRS_HIP_OK;
  if (cap < t.nblk || !max_freqs || !min_norms) return IRS_HIP_EINVAL;
  if (const int rc = prepare_blockmax(seg)) return rc;
  if (!rt::d2h(max_freqs, seg->d_blk_maxf.as<uint32_t>() + t.dir_off, size_t(t.nblk) * 4, nullptr) ||
      !rt::d2h(min_norms, seg->d_blk_minn.as<uint32_t>() + t.dir_off, size_t(t.nblk) * 4, nullptr) ||
      !rt::sync(nullptr))
    return IRS_HIP_EHIP;
  return IRS_HIP_OK;
}

static int segment_wand_source_impl(irs_hip_segment* seg, uint64_t* from_index, uint64_t* total) {
  if (!seg) return IRS_HIP_EINVAL;
  if (!rt::set_device(seg->device)) return IRS_HIP_EHIP;
  if (const int rc = prepare_blockmax(seg)) return rc;
  if (from_index) *from_index = seg->wand_from_index;
  if (total) *total = seg->total_blocks;
  return IRS_HIP_OK;
}
}  // namespace
