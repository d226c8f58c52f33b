// Host side of the C ABI: running a plan -- kernel sequencing on the context's stream, the per-context
// switches, the token pool, per-kernel timing, results.
#include "zh_host.h"

// A timing event in front of the launch `name` on `stream` (profiled plans)
static void prof_mark(zh_plan* p, ProfLane& lane, hipStream_t stream, const char* name) {
  if (!p->profiling) return;
  size_t i = lane.names.size();
  if (lane.events.size() <= i) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) {  // no timing rather than a failed run
      p->profiling = false;
      return;
    }
    lane.events.push_back(e);
  }
  if (hipEventRecord(lane.events[i], stream) != hipSuccess) {
    p->profiling = false;
    return;
  }
  lane.names.push_back(name);
}
static void prof_mark(zh_plan* p, const char* name) { prof_mark(p, p->k_main, p->ctx->stream, name); }

extern "C" void zh_plan_set_profiling(zh_plan* plan, int on) {
  if (plan) plan->profiling = on != 0;
}

extern "C" int zh_plan_kernel_times(zh_plan* p, const char** names, float* ms, int max_entries) {
  if (!p || !p->profiling || p->k_main.names.size() < 2) return 0;
  if (hipStreamSynchronize(p->ctx->stream) != hipSuccess) return 0;
  int cnt = 0;
  // the second stream's launches last, each as long as it took beside the first's (the checksum of a compress run
  // beside "zh_huffman_kernel", the second half of an uncompress batch beside the first half's writer)
  for (const ProfLane* lane : {&p->k_main, &p->k_side})
    for (size_t i = 0; i + 1 < lane->names.size() && cnt < max_entries; i++) {
      float t = 0;
      if (hipEventElapsedTime(&t, lane->events[i], lane->events[i + 1]) != hipSuccess) break;
      names[cnt] = lane->names[i];  // the marker recorded BEFORE a launch carries its name
      ms[cnt] = t;
      cnt++;
    }
  return cnt;
}

extern "C" void zh_plan_destroy(zh_plan* p) {
  if (!p) return;
  // (nothing useful can be done about a failure while tearing down)
  (void)hipSetDevice(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);
  if (p->ctx->aux_stream) (void)hipStreamSynchronize(p->ctx->aux_stream);  // (joined by every run; cheap when idle)
  if (p->l1_pool_own) (void)hipFree(p->l1_pool_own);  // (not from the context's cache)
  for (const ProfLane* lane : {&p->k_main, &p->k_side})
    for (auto e : lane->events) (void)hipEventDestroy(e);
  delete p;  // (its device memory goes back to the context's cache with its members)
}


// ZH_INFLATE=serial keeps every stream on the two-wave serial decoder (zh_inflate.hip); the
// default decodes a stream's Huffman codes in parallel (zh_inflate_split.hip).  Sizing passes and
// the block-parallel form of one stream always use the serial kernel.
bool inflate_split_enabled(const zh_ctx* ctx) {
  static const bool on = [] {
    const char* e = getenv("ZH_INFLATE");
    return !(e && strcmp(e, "serial") == 0);
  }();
  return ctx->inflate_mode < 0 ? on : ctx->inflate_mode == 0;
}
// The context's second stream and its two events, made when first asked for.  Anything that fails leaves the work in
// line on the context's stream.
static bool second_stream(zh_ctx* ctx) {
  if (!ctx->aux_stream) {
    if (hipStreamCreate(&ctx->aux_stream) != hipSuccess) {
      ctx->aux_stream = nullptr;
      (void)hipGetLastError();
      return false;
    }
  }
  if (!ctx->aux_fork && hipEventCreate(&ctx->aux_fork) != hipSuccess) ctx->aux_fork = nullptr;
  if (!ctx->aux_join && hipEventCreate(&ctx->aux_join) != hipSuccess) ctx->aux_join = nullptr;
  return ctx->aux_fork && ctx->aux_join;
}
// ZH_CHECKSUM_ASIDE=0 keeps a compress run's checksum kernels in line on the context's stream (measurement); it says
// nothing about the uncompress batch's two halves, which have their own switch (ZH_INFLATE_HALVES)
static bool checksum_aside(zh_ctx* ctx) {
  static const bool on = [] {
    const char* e = getenv("ZH_CHECKSUM_ASIDE");
    return !(e && strcmp(e, "0") == 0);
  }();
  return on && second_stream(ctx);
}
// Work beside a run on the context's second stream: fork() puts that stream behind what the run's stream `s` holds so
// far, mark() is prof_mark for it (the plan's side lane), done() closes what join() then makes `s` wait for.
// Work that was forked is joined on every way out of a run: an early return (a failed HIP call between fork and
// join) must not leave kernels of the second stream reading the caller's buffers unordered with the caller's stream
// -- the caller may free or reuse them as soon as its own stream has drained.
namespace {
struct SideLane {
  zh_plan* p;
  zh_ctx* ctx;
  hipStream_t s, side;
  bool forked = false;
  SideLane(zh_plan* plan, hipStream_t s) : p(plan), ctx(plan->ctx), s(s), side(plan->ctx->aux_stream) {}
  int fork() {
    side = ctx->aux_stream;
    ZH_HIP(ctx, hipEventRecord(ctx->aux_fork, s));
    ZH_HIP(ctx, hipStreamWaitEvent(side, ctx->aux_fork, 0));
    forked = true;
    return ZH_OK;
  }
  void mark(const char* name) { prof_mark(p, p->k_side, side, name); }
  int done() {
    mark("end");
    ZH_HIP(ctx, hipEventRecord(ctx->aux_join, side));
    return ZH_OK;
  }
  int join() {
    ZH_HIP(ctx, hipStreamWaitEvent(s, ctx->aux_join, 0));
    forked = false;
    return ZH_OK;
  }
  ~SideLane() {
    if (!forked) return;
    if (hipEventRecord(ctx->aux_join, ctx->aux_stream) != hipSuccess ||
        hipStreamWaitEvent(s, ctx->aux_join, 0) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipStreamSynchronize(ctx->aux_stream);
    }
  }
};
}  // namespace
#define ZH_TRY(call)                  \
  do {                                \
    if (const int st_ = (call)) return st_; \
  } while (0)
// ZH_L1_ORDER=0: fragments as numbered in every run (measurement: what a plan's first run costs)
static bool l1_longest_first() {
  static const bool on = [] {
    const char* e = getenv("ZH_L1_ORDER");
    return !(e && strcmp(e, "0") == 0);
  }();
  return on;
}
// The exact BestSpeed matcher of a compress plan on the context's stream (zh_l1_match.hip).  Its mixed launch is two
// kernels that share the fragments: the ordering and the counter in front of the fork, the LDS-table waves on the
// second stream beside the pooled ones, and the join behind both -- whatever follows (the code builder reads every
// fragment's histograms) sees all of it, and the main lane's interval of the matcher covers both kernels; the second
// stream's gets no entry of its own in zh_plan_kernel_times.  `use_order`: the cheapest fragments of the last run last.
int run_l1_match(zh_plan* p, const uint8_t* d_src, bool use_order) {
  zh_ctx* ctx = p->ctx;
  hipStream_t s = ctx->stream;
  const ZhCompressArgs& a = p->ca;
  const int huffman_only = p->level == -2;
  const ZhL1Launch l = zh_l1_match_prepare(s, a.nfrags, p->l1_counter, p->l1_cost, p->l1_order, p->l1_hist, use_order,
                                           second_stream(ctx));
  SideLane aux(p, s);
  if (l.pooled && l.lds) {
    ZH_TRY(aux.fork());
    zh_launch_l1_match(aux.side, d_src, a, huffman_only, p->l1_tables, p->l1_counter, p->l1_cost, l, 1);
    ZH_HIP(ctx, hipEventRecord(ctx->aux_join, aux.side));
    zh_launch_l1_match(s, d_src, a, huffman_only, p->l1_tables, p->l1_counter, p->l1_cost, l, 0);
    ZH_TRY(aux.join());
  } else {
    zh_launch_l1_match(s, d_src, a, huffman_only, p->l1_tables, p->l1_counter, p->l1_cost, l, l.lds != 0);
  }
  ZH_HIP(ctx, hipGetLastError());
  static const bool trace = getenv("ZH_TRACE") != nullptr;
  if (trace && a.nfrags) {  // (waits for the run: a tuning aid)
    uint32_t c[3] = {0, 0, 0};
    ZH_HIP(ctx, hipMemcpyAsync(c, p->l1_counter, sizeof(c), hipMemcpyDeviceToHost, s));
    ZH_HIP(ctx, hipStreamSynchronize(s));
    fprintf(stderr, "zippy_hip: exact matcher: %u pooled waves took %u fragments, %u LDS-table waves %u, of %u\n", l.pooled,
            c[1], l.lds, c[2], a.nfrags);
  }
  return ZH_OK;
}

// BestSpeed parse: 0 the reference's (snappy.nim:12-136, byte-identical streams), 1 the parallel
// parse of zh_l1p_match.hip (valid streams of about the same size, not the reference's bytes)
bool l1_parallel(const zh_ctx* ctx) {
  static const bool on = [] {
    const char* e = getenv("ZH_L1_PARSE");
    return e && strcmp(e, "parallel") == 0;
  }();
  return ctx->l1_parse < 0 ? on : ctx->l1_parse == 1;
}
extern "C" void zh_set_l1_parse(zh_ctx* ctx, int mode) {
  if (ctx) ctx->l1_parse = mode < 0 ? -1 : mode ? 1 : 0;
}
extern "C" void zh_set_inflate_mode(zh_ctx* ctx, int mode) {
  if (ctx) ctx->inflate_mode = mode < 0 ? -1 : mode ? 1 : 0;
}
// the token pool of a plan, allocated when it first runs in split mode; a failed allocation
// (it is several times the output) sends the plan to the serial kernel for good
bool plan_token_pool(zh_plan* p) {
  if (!p->tok_pool) {
    if (p->tok_failed || !p->tok_words) return false;
    if (dev_alloc(p->ctx, p->tok_own, p->tok_words * 4) != hipSuccess) {
      (void)hipGetLastError();
      p->tok_failed = true;
      // not an error (the serial decoder gives the same bytes), but several times slower: leave a note
      p->ctx->last_error = "note: no memory for a token pool of " + std::to_string(p->tok_words * 4) +
                           " bytes; this plan decodes with the serial kernel (zh_inflate_kernel)";
      if (getenv("ZH_TRACE")) fprintf(stderr, "zippy_hip: %s\n", p->ctx->last_error.c_str());
      return false;
    }
    p->tok_pool = p->tok_own.p;
  }
  if (p->segmented && !p->sg_sym.p) {  // without its buffers the plan simply is not segmented
    if (dev_alloc(p->ctx, p->sg_sym, p->sg_sym_count * 2) != hipSuccess ||
        dev_alloc(p->ctx, p->sg_windows, (size_t)p->sg.nsegs * 32768u) != hipSuccess ||
        dev_alloc(p->ctx, p->sg_winsym, (size_t)p->sg.nsegs * 65536u) != hipSuccess) {
      (void)hipGetLastError();
      p->sg_sym.release();
      p->sg_windows.release();
      p->sg_winsym.release();
      p->segmented = false;
      p->ctx->last_error = "note: no memory for the segment-wise decode's buffers; large streams of this plan "
                           "are decoded by one workgroup each";
      if (getenv("ZH_TRACE")) fprintf(stderr, "zippy_hip: %s\n", p->ctx->last_error.c_str());
    } else {
      p->sg.sym = p->sg_sym.p;
      p->sg.windows = p->sg_windows.p;
      p->sg.winsym = p->sg_winsym.p;
    }
  }
  return true;
}
// A token pool that outlives the plan and is shared with other plans whose kernels run on the same
// stream one after the other (the pool is scratch of a run: tokens kernel -> writer).
void plan_lend_token_pool(zh_plan* p, uint32_t* pool, uint64_t words) {
  if (p->tok_pool || p->tok_failed || !p->tok_words || p->tok_words > words) return;
  p->tok_pool = pool;
}

// ZH_TRACE_SEG: why a large stream was not decoded segment-wise (the run waits for the chain kernel and reads its
// verdicts back; a stream whose chain does not hold is decoded by one workgroup, correctly and slowly)
static void seg_trace(zh_plan* p, hipStream_t s) {
  const ZhSegArgs& g = p->sg;
  if (hipStreamSynchronize(s) != hipSuccess) return;
  std::vector<uint32_t> first(g.nstreams + 1), go(g.nstreams), ok(g.nstreams), nchain(g.nstreams);
  (void)hipMemcpy(first.data(), g.first_seg, first.size() * 4, hipMemcpyDeviceToHost);
  (void)hipMemcpy(go.data(), g.go, go.size() * 4, hipMemcpyDeviceToHost);
  (void)hipMemcpy(ok.data(), g.stream_ok, ok.size() * 4, hipMemcpyDeviceToHost);
  (void)hipMemcpy(nchain.data(), g.nchain, nchain.size() * 4, hipMemcpyDeviceToHost);
  {
    std::vector<uint32_t> cn(g.nfind);
    (void)hipMemcpy(cn.data(), g.cand_n, cn.size() * 4, hipMemcpyDeviceToHost);
    uint64_t total = 0, over = 0, most = 0;
    for (uint32_t c : cn) {
      total += c;
      over += c > 256u;
      most = std::max<uint64_t>(most, c);
    }
    fprintf(stderr, "zippy_hip: %u search batches of 65536 bits: %llu candidates for a block start, %llu at most, %llu batches with more than the queue's 256\n",
            g.nfind, (unsigned long long)total, (unsigned long long)most, (unsigned long long)over);
  }
  for (uint32_t i = 0; i < g.nstreams; i++) {
    const uint32_t n = first[i + 1] - first[i];
    if (!n) continue;
    fprintf(stderr, "zippy_hip: stream %u: %u segments, go %u, chain holds %u, %u on it\n", i, n, go[i], ok[i], nchain[i]);
    if (ok[i]) continue;
    std::vector<uint64_t> nominal(n), start(n), end(n), out(n), cap(n), shdr(n);
    std::vector<int32_t> st(n);
    std::vector<uint32_t> fin(n), sub(n);
    (void)hipMemcpy(nominal.data(), g.nominal_bit + first[i], n * 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(start.data(), g.start_bit + first[i], n * 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(end.data(), g.end_bit + first[i], n * 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(out.data(), g.seg_out + first[i], n * 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(cap.data(), g.eff_tok_cap + first[i], n * 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(shdr.data(), g.sub_hdr + first[i], n * 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(st.data(), g.seg_status + first[i], n * 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(fin.data(), g.final_block + first[i], n * 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(sub.data(), g.is_sub + first[i], n * 4, hipMemcpyDeviceToHost);
    // follow the chain the way zh_seg_chain_kernel does, and say where it ends
    uint64_t want = start[0];
    uint32_t k = 0, links = 0, none = 0, bad = 0;
    for (uint32_t j = 0; j < n; j++) {
      none += start[j] == ~0ull;
      bad += start[j] != ~0ull && st[j] != 0;
    }
    fprintf(stderr, "  %u segments without a start, %u with a failed decoder\n", none, bad);
    while (k < n) {
      while (k < n && start[k] != want) k++;
      if (k == n) break;
      links++;
      if (st[k] != 0 || fin[k]) break;
      want = end[k];
      k++;
    }
    const uint32_t lo = k < n ? k : 0;
    fprintf(stderr, "  chain: %u links, %s; wanted bit %llu\n", links,
            k == n ? "no segment starts where the last one stopped" : st[k] ? "a decoder failed" : "reached the last block",
            (unsigned long long)want);
    uint32_t near = 0;
    while (near + 1 < n && nominal[near + 1] <= want) near++;
    for (uint32_t j = (k == n ? near : lo) > 2 ? (k == n ? near : lo) - 2 : 0; j < n && j < (k == n ? near : lo) + 4; j++)
      fprintf(stderr, "  seg %u: nominal %llu start %lld (sub %u of the block at %lld) end %llu status %d final %u out %llu tokens' room %llu\n", j,
              (unsigned long long)nominal[j], (long long)start[j], sub[j], (long long)shdr[j], (unsigned long long)end[j], st[j], fin[j],
              (unsigned long long)out[j], (unsigned long long)cap[j]);
  }
}

// A ranges plan (zh_ranges.hip), group by group through the scratch: the blocks that lie wholly inside their ranges
// decode straight into the slots, the edge blocks into scratch, from where the clips take what belongs to the ranges;
// the reduce kernel folds the blocks' results into the ranges' once every group is through.
static int run_ranges(zh_plan* p, const uint8_t* d_src, uint8_t* d_dst) {
  zh_ctx* ctx = p->ctx;
  hipStream_t s = ctx->stream;
  const ZhRangesPlan& R = *p->rg;
  const ZhRangesArgs& a = R.a;
  for (const ZhRangesPlan::Group& g : R.groups) {
    const uint32_t sc0 = R.n_in_place + g.sc0;
    if (g.nip) ZH_HIP(ctx, hipMemsetAsync(a.blk_status + g.ip0, 0, (size_t)g.nip * 4, s));
    if (g.nsc) ZH_HIP(ctx, hipMemsetAsync(a.blk_status + sc0, 0, (size_t)g.nsc * 4, s));
    prof_mark(p, "zh_inflate_kernel");
    zh_launch_inflate(s, d_src, d_dst,
                      block_decoder_args(a.bufs + g.ip0, a.start_bit + g.ip0, g.nip, a.blk_len + g.ip0, a.blk_status + g.ip0));
    prof_mark(p, "zh_inflate_kernel");
    zh_launch_inflate(s, d_src, R.scratch.p,
                      block_decoder_args(a.bufs + sc0, a.start_bit + sc0, g.nsc, a.blk_len + sc0, a.blk_status + sc0));
    prof_mark(p, "zh_range_clip_kernel");
    zh_launch_range_clip(s, R.scratch.p, d_dst, a.clips + g.clip0, g.nclip);
    ZH_HIP(ctx, hipGetLastError());
  }
  prof_mark(p, "zh_ranges_reduce_kernel");
  zh_launch_ranges_reduce(s, a);
  prof_mark(p, "end");
  ZH_HIP(ctx, hipGetLastError());
  ctx->rg_uploaded = 0;
  ctx->rg_in_place = R.n_in_place;
  ctx->rg_via_scratch = R.n_scratch;
  return ZH_OK;
}

static int run_compress(zh_plan* p, const uint8_t* d_src, uint8_t* d_dst) {
  zh_ctx* ctx = p->ctx;
  hipStream_t s = ctx->stream;
  SideLane aux(p, s);
  const ZhCompressArgs& a = p->ca;
  const int want_crc = p->fmt == ZH_DF_GZIP || p->force_crc, want_adler = p->fmt == ZH_DF_ZLIB;
  // zh_emit_kernel and the layout kernels address the output as aligned 32-bit words.  Nothing is cleared beforehand:
  // every word that is OR-ed into is zeroed by the layout kernels first, everything else is stored whole (zh_huffman.hip)
  if ((uintptr_t)d_dst & 3u) return ZH_ERR_ARGUMENT;
  if (p->level == 1 && l1_parallel(ctx)) {
    prof_mark(p, "zh_l1p_match_kernel");
    zh_launch_l1p_match(s, d_src, a, p->l1_tables, p->l1_counter);
  } else if (p->level == 1 || p->level == -2) {
    prof_mark(p, "zh_l1_match_kernel");
    // (from the second run on the cheapest fragments -- by what they cost the run before -- are handed out last)
    ZH_TRY(run_l1_match(p, d_src, p->l1_runs > 0 && l1_longest_first()));
    p->l1_runs++;
  } else if (p->level != 0) {
    const int* cfg = kChainConfig[p->level == -1 ? 6 : p->level];
    if (p->chain_best_dirty)
      ZH_HIP(ctx, hipMemsetAsync(p->chain_best, 0, p->chain_scratch_frags * (size_t)ZH_FRAG_SIZE * 4u, s));
    p->chain_best_dirty = true;
    for (const auto& r : p->chain_ranges) {  // (one range unless the scratch budget says otherwise)
      ZhCompressArgs ar = a;
      ar.first_block = r.b0;
      ar.nblocks = r.nb;
      ar.first_frag = r.f0;
      ar.nfrags = r.nf;
      prof_mark(p, "zh_chain_prev_kernel");
      zh_launch_chain_prev(s, d_src, ar, p->head_scratch, p->chain_prev, p->chain_best, p->ctx->chain_links_serial ? 1 : 0, cfg[0]);
      ZH_HIP(ctx, hipGetLastError());
      prof_mark(p, "zh_chain_walk_kernel");
      zh_launch_chain_search(s, d_src, ar, cfg[0], cfg[1], cfg[2], p->chain_prev, p->chain_best, p->ctx->chain_links_serial ? 1 : 0);
      prof_mark(p, "zh_chain_select_kernel");
      zh_launch_chain_select(s, d_src, ar, cfg[0], cfg[1], cfg[2], p->chain_prev, p->chain_best, p->ctx->chain_links_serial ? 1 : 0);
      ZH_HIP(ctx, hipGetLastError());
    }
    p->chain_best_dirty = false;  // (every launch was accepted: the links kernel hands best[] back cleared)
    prof_mark(p, "zh_frag_stats_kernel");
    zh_launch_frag_stats(s, d_src, a);
  }
  // The checksum of the source and the blocks' code builder need nothing from each other and wait for different
  // things -- the one for the LDS (its table look-ups) on every CU, the other, a lane a block, for its own chain of
  // dependent instructions --: side by side, the checksum on the context's second stream, forked behind the match
  // finder (beside THAT it only costs) and joined in front of the layout, which writes the trailer.
  p->k_side.names.clear();
  bool trailer_late = false;
  if (want_crc || want_adler) {
    const bool aside = checksum_aside(ctx);
    if (aside) ZH_TRY(aux.fork());
    const hipStream_t cs = aside ? aux.side : s;
    auto mark = [&](const char* name) { aside ? aux.mark(name) : prof_mark(p, name); };
    mark("zh_checksum_pieces_kernel");
    zh_launch_checksum_pieces(cs, ctx->cktabs, d_src, p->d_pieces, p->npieces, nullptr, want_crc,
                              want_adler, p->piece_crc, p->piece_adler, p->piece_len);
    mark("zh_checksum_combine_kernel");
    zh_launch_checksum_combine(cs, ctx->cktabs, p->d_bufs, (uint32_t)p->n, p->piece_crc, p->piece_adler,
                               p->piece_len, want_crc, want_adler, p->buf_crc, p->buf_adler);
    if (aside) ZH_TRY(aux.done());
    // (the trailer is all that needs the checksum: in large batches it is written behind the emission -- a kernel of
    // its own --, and the checksum has the emission to run beside as well: it takes three times as long there, the
    // emission 5 % longer, and the pair ends 0.25 ms sooner)
    trailer_late = aside && p->trailer_late;
  }
  prof_mark(p, "zh_huffman_kernel");
  // (contract mode -- zh_set_l1_parse(ctx, 1), BestSpeed only -- also builds the block's codes without the
  // replay of the reference's heap: optimal codes, other tie-breaks)
  zh_launch_huffman(s, a, p->level == 1 && l1_parallel(ctx) ? 1 : 0);
  if (aux.forked && !trailer_late) ZH_TRY(aux.join());
  prof_mark(p, "zh_layout_kernel");
  zh_launch_layout(s, d_dst, a, p->buf_crc, p->buf_adler, trailer_late ? 0 : 1);
  prof_mark(p, "zh_emit_kernel");
  // (the exact BestSpeed parse and level -2 have left their coverage bitmaps for it; ZH_EMIT_COVER=0: measurement)
  static const bool cover_ok = [] { const char* e = getenv("ZH_EMIT_COVER"); return !(e && strcmp(e, "0") == 0); }();
  zh_launch_emit(s, d_src, d_dst, a, cover_ok && ((p->level == 1 && !l1_parallel(ctx)) || p->level == -2) ? 1 : 0);
  if (trailer_late) {
    prof_mark(p, "zh_trailer_kernel");
    ZH_TRY(aux.join());
    zh_launch_trailer(s, d_dst, a, p->buf_crc, p->buf_adler);
  }
  prof_mark(p, "end");
  return ZH_OK;
}

// A handful of large streams: many workgroups per stream (zh_inflate_seg.hip); streams whose chain of segments does
// not hold are left to the ordinary kernels (the caller's, which skip the others).  A sizing pass stops behind the
// chain kernel, which knows the output size by then.
static void run_segmented(zh_plan* p, const uint8_t* d_src, uint8_t* d_dst) {
  zh_ctx* ctx = p->ctx;
  hipStream_t s = ctx->stream;
  const ZhInflateArgs& a = p->ia;
  prof_mark(p, "zh_seg_find_kernel");
  zh_launch_seg_find(s, d_src, a, p->sg);
  prof_mark(p, "zh_seg_check_kernel");
  zh_launch_seg_check(s, d_src, a, p->sg);
  if (p->sg_fake_start != ~0ull) zh_launch_seg_fake_start(s, p->sg, p->sg_fake_start);
  prof_mark(p, "zh_seg_substart_kernel");
  zh_launch_seg_tokens(s, d_src, a, p->tok_pool, p->sg, 0);
  zh_launch_seg_decide(s, a, p->sg, 0);
  prof_mark(p, "zh_seg_tokens_kernel");
  zh_launch_seg_tokens(s, d_src, a, p->tok_pool, p->sg, 1);
  prof_mark(p, "zh_seg_chain_kernel");
  zh_launch_seg_chain(s, a, p->sg, 0);
  // a chain broken by found starts that were none: once more without them (streams whose chain holds sit it out)
  for (int round = 0; round < p->sg_repair_rounds; round++) {
    prof_mark(p, "zh_seg_repair_kernel");
    zh_launch_seg_repair(s, a, p->sg);
    zh_launch_seg_tokens(s, d_src, a, p->tok_pool, p->sg, 4);
    zh_launch_seg_decide(s, a, p->sg, 1);
    zh_launch_seg_tokens(s, d_src, a, p->tok_pool, p->sg, 5);
    zh_launch_seg_chain(s, a, p->sg, 1);
  }
  zh_launch_seg_stats(s, p->sg, ctx->d_seg_stats);  // (the context's two counters: made and zeroed by zh_create)
  if (p->sg_trace) seg_trace(p, s);
  if (a.count_only) return;
  prof_mark(p, "zh_seg_write_kernel");
  zh_launch_seg_write(s, d_src, a, p->tok_pool, p->sg);
  prof_mark(p, "zh_seg_windows_kernel");
  zh_launch_seg_windows(s, a, p->sg);
  prof_mark(p, "zh_seg_finish_kernel");
  zh_launch_seg_finish(s, d_dst, a, p->sg);
}

static int run_uncompress(zh_plan* p, const uint8_t* d_src, uint8_t* d_dst) {
  zh_ctx* ctx = p->ctx;
  hipStream_t s = ctx->stream;
  const ZhInflateArgs& a = p->ia;
  prof_mark(p, "zh_unwrap_kernel");
  zh_launch_unwrap(s, d_src, a);
  // (an index build, zh_seek.hip, records its points in the tokens kernel: the split decode whatever the switch says)
  const ZhRecArgs* const rec = p->rec.points ? &p->rec : nullptr;
  const bool split_ok = !p->indexed && (inflate_split_enabled(ctx) || rec) && plan_token_pool(p);
  const bool split = split_ok && !a.count_only;
  ZhInflateArgs a1 = a;
  // both checksums: with dfDetect the format is only known per stream on the device
  const int want_crc = p->fmt == ZH_DF_GZIP || p->fmt == ZH_DF_DETECT || p->force_crc;
  const int want_adler = p->fmt == ZH_DF_ZLIB || p->fmt == ZH_DF_DETECT;
  uint32_t ck_done = 0;  // checksum pieces already taken care of (the first half's, below)
  if (split_ok && p->segmented) {
    run_segmented(p, d_src, d_dst);
    a1.skip = p->sg.stream_ok;
  }
  if (p->indexed) {
    prof_mark(p, "zh_inflate_kernel");
    ZH_HIP(ctx, hipMemsetAsync(p->seg.status, 0, (size_t)p->seg.nbufs * 4, s));
    zh_launch_inflate(s, d_src, d_dst, p->seg);
    prof_mark(p, "zh_segments_reduce_kernel");
    zh_launch_segments_reduce(s, p->seg, a);
  } else if (split) {
    // two kernels: tokens (parallel over each stream), then bytes (zh_inflate_split.hip)
    p->k_side.names.clear();
    if (p->tok_groups.size() <= 1 && p->halves_min >= 2u && a1.nbufs >= p->halves_min && second_stream(ctx)) {
      // Two halves, the second on the context's second stream: 4096 workgroups are 3.2 rounds of the machine for
      // either kernel, and both wait more than they work -- side by side a half's writer fills what
      // the other half's tokens kernel leaves idle, and only the last tail is nobody's to fill (own streams 20.8 ->
      // 19.7 ms, zlib level-6 members 24.3 -> 23.4; three and four parts: slower).
      // Kernel times: both halves' launches are reported, each as long as it took BESIDE the other.
      ZhInflateArgs ah[2] = {a1, a1};
      ah[0].nbufs = a1.nbufs / 2u;
      ah[1].first_buf = a1.first_buf + ah[0].nbufs;
      ah[1].nbufs = a1.nbufs - ah[0].nbufs;
      SideLane half(p, s);
      ZH_TRY(half.fork());
      half.mark("zh_inflate_tokens_kernel");
      zh_launch_inflate_tokens(half.side, d_src, ah[1], p->tok_pool, p->tok_off, p->tok_cap, rec);
      half.mark("zh_inflate_write_kernel");
      zh_launch_inflate_write(half.side, d_src, d_dst, ah[1], p->tok_pool, p->tok_off);
      ZH_TRY(half.done());
      prof_mark(p, "zh_inflate_tokens_kernel");
      zh_launch_inflate_tokens(s, d_src, ah[0], p->tok_pool, p->tok_off, p->tok_cap, rec);
      prof_mark(p, "zh_inflate_write_kernel");
      zh_launch_inflate_write(s, d_src, d_dst, ah[0], p->tok_pool, p->tok_off);
      // (the first half's output is complete: its checksum pieces fill what the second half's tail leaves idle
      // instead of waiting for it)
      if ((want_crc || want_adler) && a1.first_buf == 0 && a1.nbufs == (uint32_t)p->n && p->half_piece) {
        prof_mark(p, "zh_checksum_pieces_kernel");
        zh_launch_checksum_pieces(s, ctx->cktabs, d_dst, p->d_pieces, p->half_piece, p->out_len, want_crc, want_adler,
                                  p->piece_crc, p->piece_adler, p->piece_len);
        ck_done = p->half_piece;
      }
      prof_mark(p, "(waiting for the other half)");
      ZH_TRY(half.join());
    } else if (p->tok_groups.size() <= 1) {
      prof_mark(p, "zh_inflate_tokens_kernel");
      zh_launch_inflate_tokens(s, d_src, a1, p->tok_pool, p->tok_off, p->tok_cap, rec);
      prof_mark(p, "zh_inflate_write_kernel");
      zh_launch_inflate_write(s, d_src, d_dst, a1, p->tok_pool, p->tok_off);
    } else {
      for (const auto& g : p->tok_groups) {  // the pool holds a group's records at a time
        ZhInflateArgs ag = a1;
        ag.first_buf = g.first;
        ag.nbufs = g.second;
        prof_mark(p, "zh_inflate_tokens_kernel");
        zh_launch_inflate_tokens(s, d_src, ag, p->tok_pool, p->tok_off, p->tok_cap, rec);
        prof_mark(p, "zh_inflate_write_kernel");
        zh_launch_inflate_write(s, d_src, d_dst, ag, p->tok_pool, p->tok_off);
      }
    }
  } else if (a.count_only && !p->indexed && inflate_split_enabled(ctx)) {
    // a sizing pass: the tokens kernel without its records (the serial decoder took several times the decode itself)
    prof_mark(p, "zh_inflate_tokens_kernel");
    zh_launch_inflate_count(s, d_src, a1);
  } else {
    prof_mark(p, "zh_inflate_kernel");
    zh_launch_inflate(s, d_src, d_dst, a1);
  }
  if (!a.count_only && (want_crc || want_adler)) {
    prof_mark(p, "zh_checksum_pieces_kernel");
    zh_launch_checksum_pieces(s, ctx->cktabs, d_dst, p->d_pieces + ck_done, p->npieces - ck_done, p->out_len,
                              want_crc, want_adler, p->piece_crc + ck_done, p->piece_adler + ck_done,
                              p->piece_len + ck_done);
    prof_mark(p, "zh_checksum_combine_kernel");
    zh_launch_checksum_combine(s, ctx->cktabs, p->d_bufs, (uint32_t)p->n, p->piece_crc, p->piece_adler,
                               p->piece_len, want_crc, want_adler, p->buf_crc, p->buf_adler);
    prof_mark(p, "zh_verify_kernel");
    zh_launch_verify(s, a, p->buf_crc, p->buf_adler);
  }
  prof_mark(p, "end");
  return ZH_OK;
}

extern "C" int zh_plan_run(zh_plan* p, const void* d_src_v, void* d_dst_v) {
  if (!p) return ZH_ERR_ARGUMENT;
  zh_ctx* ctx = p->ctx;
  const uint8_t* d_src = (const uint8_t*)d_src_v;
  uint8_t* d_dst = (uint8_t*)d_dst_v;
  p->k_main.names.clear();
  if (!p->n) return ZH_OK;
  // (a caller that drives two contexts' plans from one thread: the launches below go to the current device)
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  if (p->rg) return run_ranges(p, d_src, d_dst);
  ZH_TRY(p->is_compress ? run_compress(p, d_src, d_dst) : run_uncompress(p, d_src, d_dst));
  ZH_HIP(ctx, hipGetLastError());
  return ZH_OK;
}

extern "C" int zh_plan_results(zh_plan* p, uint64_t* out_lens, int32_t* statuses) {
  if (!p) return ZH_ERR_ARGUMENT;
  zh_ctx* ctx = p->ctx;
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  if (out_lens) ZH_HIP(ctx, hipMemcpyAsync(out_lens, p->out_len, p->n * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (statuses) ZH_HIP(ctx, hipMemcpyAsync(statuses, p->status, p->n * 4, hipMemcpyDeviceToHost, ctx->stream));
  ZH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ZH_OK;
}
extern "C" int zh_debug_segment_stats(zh_ctx* ctx, uint64_t* cut, uint64_t* held) {
  if (!ctx) return ZH_ERR_ARGUMENT;
  uint64_t h[2] = {0, 0};
  if (ctx->d_seg_stats) {
    ZH_HIP(ctx, hipSetDevice(ctx->device));
    ZH_HIP(ctx, hipMemcpyAsync(h, ctx->d_seg_stats, 16, hipMemcpyDeviceToHost, ctx->stream));
    ZH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (cut) *cut = h[0];
  if (held) *held = h[1];
  return ZH_OK;
}
extern "C" int zh_plan_request_crc32(zh_plan* p, int on) {
  if (!p || p->rg) return ZH_ERR_ARGUMENT;
  p->force_crc = on != 0;
  return ZH_OK;
}
extern "C" int zh_plan_crc32(zh_plan* p, uint32_t* crcs) {
  if (!p || !crcs || !p->buf_crc) return ZH_ERR_ARGUMENT;
  zh_ctx* ctx = p->ctx;
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  ZH_HIP(ctx, hipMemcpyAsync(crcs, p->buf_crc, p->n * 4, hipMemcpyDeviceToHost, ctx->stream));
  ZH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ZH_OK;
}
extern "C" const uint64_t* zh_plan_device_lens(zh_plan* p) { return p ? p->out_len : nullptr; }
extern "C" const int32_t* zh_plan_device_statuses(zh_plan* p) { return p ? p->status : nullptr; }
