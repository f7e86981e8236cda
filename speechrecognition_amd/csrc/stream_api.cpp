// stream_api.cpp -- the host code of streaming recognition: sr_stream_* (decode_stream_kernel over per-slot state in device memory),
// sr_bigram_stream_* (bigram_stream_kernel likewise) and the test hook sr_commit_points.  include/srgpu.h has the definitions.
//
// Compiled as part of srgpu_api.cpp's translation unit, which includes this file after the scoring and chunk helpers it uses
// (run_chunks, launch_scoring, prof_begin / prof_end, check_model).  The two kinds of set derive from StreamSet (handles.h); what touches
// only the shared members is a plain function on it and is written once: the front end, projection, transform and warp setters, the
// pipeline's plan and launch (plan_pipeline, launch_pipeline), the lifecycle (open_check, open_set, begin_set, end_check, close_slot,
// destroy_set), the ids of a call (slot_of for one, srplan::resolve_ids worded by refuse_ids for several) and the pinned job block of
// the stable and trim calls (run_block).  What needs the search is generic over the set:
// stream_precheck, stream_run, and the pushes that call them (push_rows and push_audio, which share push_tail).  The bookkeeping that
// needs no device -- slots and ids, the window checks, the block's layout -- is stream_set_plan.h.

namespace {
// an entry of a push with frames: its stream slot, the frames searched before the push, the frames in it, its first frame's row in
// the push's features
struct PushEntry { uint32_t slot; uint64_t t0, k, row0; };
// A push's pass: its F frames and its jobs staged on the device, then one chunk of run_chunks -- the frames scored into m->scores[0],
// search(chunk, table, stream) enqueuing the push's search.  feats == nullptr: work queued on the scoring stream has the frames in
// d_feats already (the audio pushes).  (Every call synchronises before it returns: the buffer is free.)
template <class Job, class Search>
int push_pass(sr_model* m, int gmm_kernel, const float* feats, uint64_t F, DevBuf<float>& d_feats, const std::vector<Job>& jobs,
              DevBuf<Job>& d_jobs, Search search) {
  HIP_TRY(d_feats.ensure((size_t)F * m->dim));
  HIP_TRY(m->scores[0].ensure((size_t)F * m->ld));
  HIP_TRY(d_jobs.ensure(jobs.size()));
  if (feats) HIP_TRY(hipMemcpyAsync(d_feats.p, feats, sizeof(float) * F * m->dim, hipMemcpyHostToDevice, m->s_gmm));
  HIP_TRY(hipMemcpyAsync(d_jobs.p, jobs.data(), sizeof(Job) * jobs.size(), hipMemcpyHostToDevice, m->s_gmm));
  return run_chunks(m, {Chunk{0, (uint32_t)jobs.size(), 0, F}},
                    [&](const Chunk&, double* table) { return launch_scoring(m, d_feats.p, F, gmm_kernel, table); }, search);
}

// the partial (after every push) or final words of the utterance in `slot`
int stream_words(sr_stream* s, uint32_t slot, uint32_t id, uint32_t* out_words, uint32_t cap, uint32_t* count) {
  *count = 0;
  if (s->slots.frames[slot] == 0) return SR_OK;  // nothing searched yet: the empty utterance's (no) words
  StreamState st;
  HIP_TRY(hipMemcpy(&st, s->state.p + slot, sizeof(st), hipMemcpyDeviceToHost));
  if (st.flags & kFlagCorrupt) return fail(SR_ECORRUPT, "stream %u: the traceback does not walk back to frame 0 (Recognizer.cpp:222-231)", id);
  if (st.count > s->slots.frames[slot]) return fail(SR_ECORRUPT, "stream %u: %u words for %llu frames", id, st.count, (unsigned long long)s->slots.frames[slot]);
  // A trimmed utterance (sr_stream_trim): the window's walk ends at the last commit point, the words before it are in the archive.
  // The reference's walk from an entry without a surviving word end reports no earlier word at all, so the archive
  // leads only where the walk started at a finite entry.
  const std::vector<uint32_t>& arch = s->archive[slot];
  size_t lead = arch.size();
  if (lead) {
    double last = 0.0;
    HIP_TRY(hipMemcpy(&last, s->tb_score.p + (size_t)slot * (s->slots.max_frames + 1) + s->slots.frames[slot], sizeof(double), hipMemcpyDeviceToHost));
    if (!(last < __builtin_huge_val())) lead = 0;
  }
  const uint64_t total = (uint64_t)lead + st.count;
  *count = (uint32_t)std::min<uint64_t>(total, 0xFFFFFFFFull);
  if (total > cap) return fail(SR_EINVAL, "stream %u: %llu words, out_words holds %u", id, (unsigned long long)total, cap);
  if (lead) memcpy(out_words, arch.data(), sizeof(uint32_t) * lead);
  if (st.count) HIP_TRY(hipMemcpy(out_words + lead, s->words.p + (size_t)slot * s->slots.max_frames, sizeof(uint32_t) * st.count, hipMemcpyDeviceToHost));
  return SR_OK;
}
// the partial (after every push) or final traceback items of the utterance in `slot`: the state record read back after its last push
int bigram_stream_items(sr_bigram_stream* s, uint32_t slot, uint32_t id, uint32_t* out_word, float* out_score, uint32_t* out_time,
                        uint32_t cap, uint32_t* count) {
  *count = 0;
  if (s->slots.frames[slot] == 0) return SR_OK;  // nothing searched yet: the empty utterance's (no) items
  if (s->failed[slot]) return fail(SR_EINTERNAL, "stream %u: a push overflowed its book", id);
  const BigramStreamState& st = s->host_state[slot];
  if (st.flags & kBgStreamCorrupt) return fail(SR_ECORRUPT, "stream %u: the book walk does not end at its start entry", id);
  *count = st.count;
  if (st.count > cap) return fail(SR_EINVAL, "stream %u: %u items, the output arrays hold %u", id, st.count, cap);
  const size_t o = (size_t)slot * (s->slots.max_frames + 1);
  if (st.count) {
    HIP_TRY(hipMemcpy(out_word, s->out_word.p + o, sizeof(uint32_t) * st.count, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_score, s->out_score.p + o, sizeof(float) * st.count, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_time, s->out_time.p + o, sizeof(uint32_t) * st.count, hipMemcpyDeviceToHost));
  }
  return SR_OK;
}

// The two stream sets' pushes behind their checks, for feature rows and audio alike.  stream_precheck: what the set itself has
// against the entries, before any launch.  stream_run: the push's F rows (feats on the host, or nullptr: already in s->feats on the
// device) scored and searched; the entries' frame counts advance.
int stream_precheck(sr_stream*, const std::vector<PushEntry>&) { return SR_OK; }
int stream_run(sr_stream* s, const std::vector<PushEntry>& entries, const float* feats, uint64_t F) {
  sr_model* m = s->model;
  const sr_lexicon* l = s->lex;
  std::vector<StreamJob> jobs;
  for (const PushEntry& e : entries) jobs.push_back({e.slot, (uint32_t)e.t0, (uint32_t)e.k, 0u, e.row0});
  int rc = push_pass(m, s->params.gmm_kernel, feats, F, s->feats, jobs, s->jobs, [&](const Chunk&, const double* table, hipStream_t st) -> int {
    StreamArgs a{};
    a.net = l->net;
    a.am_threshold = s->params.am_threshold; a.word_penalty = s->params.word_penalty;
    a.scores = table; a.ld = m->ld; a.jobs = s->jobs.p;
    a.ws = s->ws.p; a.ws_stride = decode_big_workspace(l->net.n_slots); a.state = s->state.p;
    a.tb_score = s->tb_score.p; a.tb_word = s->tb_word.p; a.tb_bkp = s->tb_bkp.p; a.tb_stride = s->slots.max_frames + 1;
    a.words = s->words.p; a.words_stride = s->slots.max_frames;
    HIP_TRY(launch_decode_stream(a, (uint32_t)jobs.size(), st));
    if (m->profiling) {
      m->prof.search_bytes += (8.0 * m->n_states + 4.0 * l->net.n_slots) * (double)F;
      m->prof.frames += F;
    }
    return SR_OK;
  });
  if (rc) return rc;
  for (const StreamJob& j : jobs) s->slots.frames[j.slot] += j.k;
  return SR_OK;
}

// per entry: the book entries the push may reach (n_book + W per frame: a frame keeps at most one word end per history)
uint64_t book_need(const sr_bigram_stream* s, const PushEntry& e) {
  return (e.t0 ? s->host_state[e.slot].n_book : 2u) + (uint64_t)s->bigram->net.n_words * e.k;
}
int stream_precheck(sr_bigram_stream* s, const std::vector<PushEntry>& entries) {
  for (const PushEntry& e : entries) {
    const uint32_t id = s->slots.id[e.slot];
    if (s->failed[e.slot]) return fail(SR_EINTERNAL, "stream id %u: an earlier push overflowed its book", id);
    const uint64_t nb = book_need(s, e);
    if (nb > 0xFFFFFFFFull)
      return fail(SR_ELIMIT, "stream id %u: this push may need %llu book entries, more than 2^32 - 1", id, (unsigned long long)nb);
  }
  return SR_OK;
}
int stream_run(sr_bigram_stream* s, const std::vector<PushEntry>& entries, const float* feats, uint64_t F) {
  sr_model* m = s->model;
  const sr_bigram* b = s->bigram;
  std::vector<BigramStreamJob> jobs;
  for (const PushEntry& e : entries) jobs.push_back({e.slot, (uint32_t)e.t0, (uint32_t)e.k, 0u, e.row0, nullptr, 0});
  // every book to at least n_book + W k entries (geometric growth; the entries so far are copied: back pointers are indices)
  for (size_t j = 0; j < jobs.size(); j++) {
    DevBuf<uint4>& bk = *s->book[jobs[j].slot];
    const uint64_t need = book_need(s, entries[j]);
    if (bk.n < need) {
      DevBuf<uint4> grown;
      HIP_TRY(grown.ensure(std::max<uint64_t>(need, std::min<uint64_t>(2 * (uint64_t)bk.n, 0xFFFFFFFFull))));
      if (jobs[j].t0) HIP_TRY(hipMemcpy(grown.p, bk.p, sizeof(uint4) * s->host_state[jobs[j].slot].n_book, hipMemcpyDeviceToDevice));
      bk.swap(grown);
    }
    jobs[j].book = bk.p;
    jobs[j].book_cap = bk.n;
  }
  int rc = push_pass(m, s->params.gmm_kernel, feats, F, s->feats, jobs, s->jobs, [&](const Chunk&, const double* table, hipStream_t stream) -> int {
    BigramStreamArgs a{};
    BigramArgs& ba = a.a;
    ba = b->net;
    ba.scores = table; ba.ld = m->ld;
    ba.ac_pruning = s->params.acoustic_pruning; ba.lm_pruning = s->params.lm_pruning;
    ba.global_states = 1;
    ba.gs_ws = s->gs_ws.p; ba.gs_ws_words = bigram_gs_ws_words(ba.n_words, ba.n_positions);
    ba.we_slot = s->we_slot.p; ba.we_bp = s->we_bp.p; ba.we_score = s->we_score.p;
    a.jobs = s->jobs.p; a.state = s->state.p; a.lsave = s->lsave.p;
    a.out_word = s->out_word.p; a.out_score = s->out_score.p; a.out_time = s->out_time.p; a.items_stride = s->slots.max_frames + 1;
    HIP_TRY(launch_bigram_stream(a, (uint32_t)jobs.size(), stream));
    if (m->profiling) {  // SURVEY 8(d)'s decoder model, 8 S + 4 P bytes per frame, as sr_recognize_bigram_corpus
      m->prof.search_bytes += (8.0 * m->n_states + 4.0 * ba.n_positions) * (double)F;
      m->prof.frames += F;
    }
    return SR_OK;
  });
  if (rc) return rc;
  std::vector<BigramStreamState> st(s->slots.max_streams);  // (one copy of every slot's 32 bytes: cheaper than one per pushed slot)
  HIP_TRY(hipMemcpy(st.data(), s->state.p, sizeof(BigramStreamState) * st.size(), hipMemcpyDeviceToHost));
  uint32_t bad = 0xFFFFFFFFu;
  for (const BigramStreamJob& j : jobs) {
    s->slots.frames[j.slot] += j.k;
    s->host_state[j.slot] = st[j.slot];
    if (st[j.slot].flags & kBgStreamOverflow) { s->failed[j.slot] = 1; bad = s->slots.id[j.slot]; }
  }
  if (bad != 0xFFFFFFFFu) return fail(SR_EINTERNAL, "stream id %u: a book append passed the capacity the host grew it to", bad);
  return SR_OK;
}

// ---- ids ------------------------------------------------------------------------------------------------------------------------------
// the slot of the one open utterance a call names
int slot_of(const StreamSet* s, uint32_t id, uint32_t* slot) {
  const int64_t at = s->slots.find(id);
  if (at < 0) return fail(SR_EINVAL, "stream id %u is not open", id);
  *slot = (uint32_t)at;
  return SR_OK;
}
// The ids of a call that names several: slots[0 .. r.entry) are set (srplan::resolve_ids).  A caller with checks of its own per entry
// runs them entry by entry up to r.entry and then refuses that entry with refuse_ids, so that the first failing check answers: in the
// words of a push ("push entry", "push") or of a stable / trim call ("entry", "call").
int refuse_ids(const srplan::IdResolution& r, const uint32_t* ids, const char* entry, const char* call) {
  if (r.fault == srplan::kIdsGood) return SR_OK;
  if (r.fault == srplan::kIdNotOpen) return fail(SR_EINVAL, "%s %u: stream id %u is not open", entry, r.entry, ids[r.entry]);
  return fail(SR_EINVAL, "%s %u: stream id %u appears twice in one %s", entry, r.entry, ids[r.entry], call);
}

// ---- the setters ------------------------------------------------------------------------------------------------------------------------
// sr_stream_set_frontend and its bigram twin.  With a projection attached the front end feeds the pipeline: any model of the
// projection's input dimension on the set's device will do.
int set_frontend(StreamSet* s, sr_frontend* fe) {
  if (!s) return fail(SR_EINVAL, "null stream set");
  for (uint32_t i = 0; i < s->slots.max_streams; i++)
    if (s->slots.open[i]) return fail(SR_EINVAL, "stream id %u is open: the front end changes only while none is", s->slots.id[i]);
  if (!fe) { s->audio.fe = nullptr; return SR_OK; }
  if (!s->pipe.projection) {
    if (fe->model != s->model) return fail(SR_EINVAL, "the front end does not belong to the stream set's model");
  } else {
    if (!fe->model || fe->model->device != s->model->device) return fail(SR_EINVAL, "the front end is not on the stream set's device");
    if (fe->model->dim != s->pipe.in_dim)
      return fail(SR_EINVAL, "the front end's rows have %u columns, the projection takes %u", fe->model->dim, s->pipe.in_dim);
  }
  if (!fe->has_mfcc) return fail(SR_EINVAL, "this front end was made without an MFCC stage: it takes cepstra only");
  int rc = check_model(s->model);
  if (rc) return rc;
  HIP_TRY(s->audio.state.ensure((size_t)s->slots.max_streams * (2 * (size_t)fe->post.deriv_step * fe->post.n_static + 1)));
  s->audio.fe = fe;
  return SR_OK;
}

// sr_stream_set_projection and its bigram twin
int set_projection(StreamSet* s, uint32_t in_dim, uint32_t context, const double* M) {
  if (!s) return fail(SR_EINVAL, "null stream set");
  for (uint32_t i = 0; i < s->slots.max_streams; i++)
    if (s->slots.open[i]) return fail(SR_EINVAL, "stream id %u is open: the projection changes only while none is", s->slots.id[i]);
  StreamPipeline& pl = s->pipe;
  const sr_frontend* fe = s->audio.fe;
  if (!M) {
    if (fe && fe->model != s->model)
      return fail(SR_EINVAL, "the attached front end does not belong to the stream set's model: detach it before the projection");
    pl.projection = false; pl.in_dim = 0; pl.context = 0;
    pl.M.release(); pl.hist.release();
    return SR_OK;
  }
  if (in_dim == 0) return fail(SR_EINVAL, "in_dim must be positive");
  const uint64_t E = (2 * (uint64_t)context + 1) * in_dim;
  if (E > 512) return fail(SR_ELIMIT, "(2 context + 1) in_dim = %llu exceeds 512 (sr_corpus_splice_transform's limit)", (unsigned long long)E);
  if (fe && fe->model->dim != in_dim)
    return fail(SR_EINVAL, "the attached front end's rows have %u columns, not in_dim = %u", fe->model->dim, in_dim);
  sr_model* m = s->model;
  if (stream_pipeline_lds_bytes(in_dim, context, m->dim, true, m->dim <= 63) > 65536)
    return fail(SR_ELIMIT, "the pipeline's LDS need exceeds 64 KB");
  int rc = check_model(m);
  if (rc) return rc;
  DevBuf<double> dM;
  DevBuf<float> hist;
  HIP_TRY(dM.upload(M, (size_t)m->dim * (E + 1)));
  HIP_TRY(hist.ensure((size_t)s->slots.max_streams * 2 * context * in_dim));
  pl.M.swap(dM); pl.hist.swap(hist);
  pl.projection = true; pl.in_dim = in_dim; pl.context = context;
  return SR_OK;
}

// sr_stream_set_transform and its bigram twin
int set_transform(StreamSet* s, uint32_t id, const double* W) {
  if (!s) return fail(SR_EINVAL, "null stream set");
  uint32_t slot = 0;
  int rc = slot_of(s, id, &slot);
  if (rc) return rc;
  if (s->audio.kind[slot] != kStreamFresh)
    return fail(SR_EINVAL, "stream id %u has been pushed to: its transform is set between begin and the first push", id);
  StreamPipeline& pl = s->pipe;
  if (!W) { pl.has_w[slot] = 0; return SR_OK; }
  sr_model* m = s->model;
  const size_t p = m->dim, n = p * (p + 1);
  if (p > 63) return fail(SR_ELIMIT, "dim %u: the transform's kernel keeps W in the LDS (max 63, as sr_corpus_transform)", m->dim);
  if ((rc = check_model(m))) return rc;
  HIP_TRY(pl.W.ensure((size_t)s->slots.max_streams * n));
  HIP_TRY(hipMemcpy(pl.W.p + (size_t)slot * n, W, sizeof(double) * n, hipMemcpyHostToDevice));
  pl.has_w[slot] = 1;
  return SR_OK;
}

// sr_stream_set_warp and its bigram twin: host state only.  sr_stream_set_frontend runs only while no id is open and every begin and end
// clears the slot's warp, so a warp never meets a front end other than the one it was checked against.
int set_warp(StreamSet* s, uint32_t id, uint32_t warp) {
  if (!s) return fail(SR_EINVAL, "null stream set");
  uint32_t slot = 0;
  const int rc = slot_of(s, id, &slot);
  if (rc) return rc;
  if (s->audio.kind[slot] != kStreamFresh)
    return fail(SR_EINVAL, "stream id %u has been pushed to: its warp is set between begin and the first push", id);
  const sr_frontend* fe = s->audio.fe;
  if (!fe) return fail(SR_EINVAL, "the stream set has no front end (sr_stream_set_frontend)");
  if (fe->n_warps == 0) return fail(SR_EINVAL, "the stream set's front end has no warps: make it with sr_frontend_create_warped");
  if (warp != SR_STREAM_NO_WARP && warp >= fe->n_warps) return fail(SR_EINVAL, "stream id %u: warp %u >= n_warps %u", id, warp, fe->n_warps);
  s->audio.warp[slot] = warp;
  return SR_OK;
}

// ---- the pipeline's part of a push ---------------------------------------------------------------------------------------------------
// Over the ids in slots[]: entry i gains k[i] input rows (finishing: none follow).  plan_pipeline: the steps of stream_pipeline_plan.h,
// where the rows they emit go in the push's output (out_off) and the entries to search.  The pipeline is active for a push when the
// set has a projection or one of the named utterances a transform; otherwise the input rows are the rows searched and no kernel of
// it runs.
struct PipelinePush {
  std::vector<srplan::PipelineStep> steps;
  std::vector<uint64_t> out_off;
  std::vector<PushEntry> entries;
  std::vector<StreamPipelineJob> jobs;  // (uploaded asynchronously: alive until the caller has synchronised)
  bool active = false;
};
void plan_pipeline(const StreamSet* s, const std::vector<uint32_t>& slots, const std::vector<uint64_t>& k, bool finishing, PipelinePush* pp) {
  const StreamPipeline& pl = s->pipe;
  const size_t n = slots.size();
  pp->steps.resize(n);
  pp->out_off.assign(n + 1, 0);
  pp->active = pl.projection;
  for (size_t i = 0; i < n; i++) {
    pp->steps[i] = srplan::plan_pipeline_step(pl.context, pl.carry[slots[i]], k[i], finishing);
    pp->out_off[i + 1] = pp->out_off[i] + pp->steps[i].rows;
    // (the pipeline counts the utterance's rows, the search its window's: sr_stream_trim)
    if (pp->steps[i].rows) pp->entries.push_back({slots[i], pp->steps[i].row0 - s->base[slots[i]], pp->steps[i].rows, pp->out_off[i]});
    if (pl.has_w[slots[i]]) pp->active = true;
  }
}
// one launch of stream_pipeline_kernel on the scoring stream: entry i's new input rows begin at row in_off[i] of pl.in (uploaded or
// written by work queued before); the rows that became ready land in s->feats.  The caller synchronises the stream.
int launch_pipeline(StreamSet* s, const std::vector<uint32_t>& slots, PipelinePush& pp, const uint64_t* in_off) {
  StreamPipeline& pl = s->pipe;
  sr_model* m = s->model;
  std::vector<StreamPipelineJob>& jobs = pp.jobs;
  for (size_t i = 0; i < slots.size(); i++) {
    const srplan::PipelineStep& st = pp.steps[i];
    if (!st.rows_in && !st.rows) continue;
    const srplan::PipelineCarry& c = pl.carry[slots[i]];
    jobs.push_back({slots[i], pl.has_w[slots[i]], (uint32_t)c.received, (uint32_t)st.rows_in, (uint32_t)st.row0, (uint32_t)st.rows,
                    in_off ? in_off[i] : 0, pp.out_off[i]});
  }
  if (jobs.empty()) return SR_OK;
  HIP_TRY(pl.jobs.ensure(jobs.size()));
  HIP_TRY(s->feats.ensure((size_t)pp.out_off.back() * m->dim));
  HIP_TRY(hipMemcpyAsync(pl.jobs.p, jobs.data(), sizeof(StreamPipelineJob) * jobs.size(), hipMemcpyHostToDevice, m->s_gmm));
  StreamPipelineArgs a{};
  a.jobs = pl.jobs.p;
  a.in_dim = pl.projection ? pl.in_dim : m->dim; a.context = pl.context; a.dim = m->dim;
  a.M = pl.projection ? pl.M.p : nullptr;
  a.W = pl.W.p;
  a.w_doubles = pl.W.p ? m->dim * (m->dim + 1) : 0;
  a.y_floats = pl.projection && pl.W.p ? stream_pipeline_group_rows() * m->dim : 0;
  a.hist = pl.hist.p; a.in = pl.in.p; a.out = s->feats.p;
  EventPair ep{};
  int rc = prof_begin(m, m->s_gmm, 1, &ep);
  if (rc) return rc;
  HIP_TRY(launch_stream_pipeline(a, (uint32_t)jobs.size(), m->s_gmm));
  return prof_end(m, m->s_gmm, &ep);
}

// ---- the pushes -----------------------------------------------------------------------------------------------------------------------
// What a push's own part hands the shared tail: the rows to search where they are still on the host (rows pushed with no pipeline in
// between), where entry i's input rows begin in the pipeline's input, and whether it queued work on the scoring stream.
struct PushFeed {
  const float* host_rows = nullptr;
  const uint64_t* in_off = nullptr;
  bool queued = false;
};
// Everything a row push and an audio push share once the named utterances' new input rows k[] are known: the pipeline's steps, the
// capacity of out_feats, the set's own checks, then feed(pp, &fd) -- the caller's last checks and its uploads and launches, which leave
// the input rows in pl.in (active pipeline), the rows to search in s->feats, or those on the host (fd.host_rows) -- the pipeline's
// launch, the set's scoring and search on the rows that became ready, the rows back to the caller and the commit of the pipeline's
// carries.  Nothing of the set changes before the launches have succeeded; the caller's own carries follow an SR_OK.
template <class Set, class Feed>
int push_tail(Set* s, const std::vector<uint32_t>& slots, const std::vector<uint64_t>& k, bool finishing, float* out_feats, uint64_t cap_rows,
              uint64_t* out_frame_off, Feed feed) {
  sr_model* m = s->model;
  const size_t n = slots.size();
  PipelinePush pp;
  plan_pipeline(s, slots, k, finishing, &pp);
  const uint64_t R = pp.out_off[n];
  if (out_feats && cap_rows < R) {
    if (out_frame_off) out_frame_off[n] = R;
    return fail(SR_EINVAL, "this push readies %llu rows, out_feats holds %llu", (unsigned long long)R, (unsigned long long)cap_rows);
  }
  int rc = stream_precheck(s, pp.entries);
  if (rc) return rc;
  PushFeed fd;
  if ((rc = feed(pp, &fd))) return rc;
  if (pp.active) {
    if ((rc = launch_pipeline(s, slots, pp, fd.in_off))) return rc;
    fd.queued = fd.queued || !pp.jobs.empty();
  }
  if (R) rc = stream_run(s, pp.entries, fd.host_rows, R);  // (a push that readies no row launches no scoring and no search)
  else if (fd.queued) HIP_TRY(hipStreamSynchronize(m->s_gmm));
  if (rc) return rc;
  if (R && out_feats) {
    if (fd.host_rows) memcpy(out_feats, fd.host_rows, sizeof(float) * (size_t)R * m->dim);
    else HIP_TRY(hipMemcpy(out_feats, s->feats.p, sizeof(float) * (size_t)R * m->dim, hipMemcpyDeviceToHost));
  }
  for (size_t i = 0; i < n; i++) s->pipe.carry[slots[i]] = pp.steps[i].next;
  if (out_frame_off) memcpy(out_frame_off, pp.out_off.data(), sizeof(uint64_t) * pp.out_off.size());
  return SR_OK;
}

// sr_stream_push_rows and its bigram twin (sr_stream_push is this without a finish and without rows back): all checks, then -- with an
// active pipeline -- the rows uploaded as the pipeline's input, else searched as they are.
template <class Set>
int push_rows(Set* s, uint32_t n, const uint32_t* ids, const float* feats, const uint64_t* frame_off, bool finishing, float* out_feats,
              uint64_t cap_rows, uint64_t* out_frame_off) {
  if (!s) return fail(SR_EINVAL, "null stream set");
  if (n == 0) {
    if (out_frame_off) out_frame_off[0] = 0;
    return SR_OK;
  }
  if (!ids || (!finishing && !frame_off)) return fail(SR_EINVAL, "null argument");
  if (frame_off && frame_off[0] != 0) return fail(SR_EINVAL, "frame_off[0] must be 0");
  const StreamSlots& sl = s->slots;
  StreamPipeline& pl = s->pipe;
  sr_model* m = s->model;
  std::vector<uint32_t> slots(n);
  std::vector<uint64_t> k(n, 0);
  const srplan::IdResolution named = srplan::resolve_ids(sl, n, ids, slots.data());
  for (uint32_t i = 0; i < named.entry; i++) {
    const uint32_t slot = slots[i];
    if (s->audio.kind[slot] >= kStreamAudio) return fail(SR_EINVAL, "push entry %u: stream id %u is fed as audio; it takes no feature rows", i, ids[i]);
    if (s->audio.warp[slot] != SR_STREAM_NO_WARP)
      return fail(SR_EINVAL, "push entry %u: stream id %u carries VTLN warp %u, which applies to audio; it takes no feature rows", i, ids[i],
                  s->audio.warp[slot]);
    if (pl.carry[slot].finished) return fail(SR_EINVAL, "push entry %u: stream id %u is finished; it takes no more rows", i, ids[i]);
    if (frame_off) {
      if (frame_off[i + 1] < frame_off[i]) return fail(SR_EINVAL, "frame_off is not ascending at entry %u", i);
      k[i] = frame_off[i + 1] - frame_off[i];
    }
    const uint64_t received = pl.carry[slot].received;
    switch (srplan::check_window(sl.max_frames, s->base[slot], received, k[i])) {
      case srplan::kWindowOverMaxFrames:
        return fail(SR_ELIMIT, "stream id %u: %llu + %llu frames exceed max_frames %llu", ids[i], (unsigned long long)(received - s->base[slot]),
                    (unsigned long long)k[i], (unsigned long long)sl.max_frames);
      case srplan::kWindowOverUtterance:
        return fail(SR_ELIMIT, "stream id %u: %llu + %llu rows exceed 2^32 - 1", ids[i], (unsigned long long)received, (unsigned long long)k[i]);
      case srplan::kWindowGood: break;
    }
  }
  int rc = refuse_ids(named, ids, "push entry", "push");
  if (rc) return rc;
  const uint64_t F = frame_off ? frame_off[n] : 0;
  rc = push_tail(s, slots, k, finishing, out_feats, cap_rows, out_frame_off, [&](const PipelinePush& pp, PushFeed* fd) -> int {
    if (F && !feats) return fail(SR_EINVAL, "null feats");
    int rc = SR_OK;
    if (!pp.active) {  // (no delay: the rows pushed are the rows searched)
      fd->host_rows = feats;
      return pp.out_off[n] ? check_model(m) : SR_OK;
    }
    if (!F && !pp.out_off[n]) return SR_OK;
    if ((rc = check_model(m))) return rc;
    const uint32_t D = pl.projection ? pl.in_dim : m->dim;
    HIP_TRY(pl.in.ensure((size_t)F * D));
    if (F) HIP_TRY(hipMemcpyAsync(pl.in.p, feats, sizeof(float) * (size_t)F * D, hipMemcpyHostToDevice, m->s_gmm));
    fd->in_off = frame_off;
    fd->queued = true;
    return SR_OK;
  });
  if (rc) return rc;
  for (uint32_t i = 0; i < n; i++) s->audio.kind[slots[i]] = kStreamRows;
  return SR_OK;
}

// sr_stream_push_audio / sr_stream_finish_audio and their bigram twins (include/srgpu.h has the definition): the steps of
// stream_audio_plan.h for every named utterance, all checks, then one launch of stream_frontend_kernel that leaves the ready rows
// in s->feats.  With an active pipeline the front end's rows are the pipeline's input instead: its steps are planned on them, its
// kernel follows the front end's on the same stream, and its rows are the ones searched.
template <class Set>
int push_audio(Set* s, uint32_t n, const uint32_t* ids, const int16_t* samples, const uint64_t* sample_off, bool finishing, float* out_feats,
               uint64_t cap_rows, uint64_t* out_frame_off) {
  if (!s) return fail(SR_EINVAL, "null stream set");
  StreamAudio& au = s->audio;
  const StreamSlots& sl = s->slots;
  sr_frontend* fe = au.fe;
  if (!fe) return fail(SR_EINVAL, "the stream set has no front end (sr_stream_set_frontend)");
  if (n == 0) {
    if (out_frame_off) out_frame_off[0] = 0;
    return SR_OK;
  }
  if (!ids || (!finishing && !sample_off)) return fail(SR_EINVAL, "null argument");
  if (sample_off && sample_off[0] != 0) return fail(SR_EINVAL, "sample_off[0] must be 0");
  const sr_mfcc_params& p = fe->mfcc;
  const uint32_t step = fe->post.deriv_step, nf = fe->post.n_static, H = 2 * step;
  sr_model* m = s->model;
  std::vector<srplan::AudioStep> steps(n);
  std::vector<uint32_t> slots(n);
  std::vector<uint64_t> row_off((size_t)n + 1, 0), rows_in(n, 0);  // (the front end's rows: the pipeline's input)
  const srplan::IdResolution named = srplan::resolve_ids(sl, n, ids, slots.data());
  for (uint32_t i = 0; i < named.entry; i++) {
    const uint32_t slot = slots[i];
    if (au.kind[slot] == kStreamRows) return fail(SR_EINVAL, "push entry %u: stream id %u is fed feature rows; it takes no audio", i, ids[i]);
    if (au.kind[slot] == kStreamAudioFinished) return fail(SR_EINVAL, "push entry %u: stream id %u is finished; it takes no more audio", i, ids[i]);
    uint64_t k = 0;
    if (sample_off) {
      if (sample_off[i + 1] < sample_off[i]) return fail(SR_EINVAL, "sample_off is not ascending at entry %u", i);
      k = sample_off[i + 1] - sample_off[i];
    }
    if (k && !samples) return fail(SR_EINVAL, "samples is null");
    const srplan::AudioCarry& c = au.carry[slot];
    // the frames the utterance's samples make, held against the window as the frames past the dropped ones: with have = base and
    // add = made - base the two checks read made - base > max_frames and made > 2^32 - 1
    const uint64_t made = srplan::audio_frames(p.window, p.shift, c.n_samples + k);
    switch (srplan::check_window(sl.max_frames, s->base[slot], s->base[slot], made - s->base[slot])) {
      case srplan::kWindowOverMaxFrames:
        return fail(SR_ELIMIT, "stream id %u: %llu + %llu samples make more than max_frames %llu frames", ids[i], (unsigned long long)c.n_samples,
                    (unsigned long long)k, (unsigned long long)sl.max_frames);
      case srplan::kWindowOverUtterance:
        return fail(SR_ELIMIT, "stream id %u: %llu + %llu samples make more than 2^32 - 1 frames", ids[i], (unsigned long long)c.n_samples,
                    (unsigned long long)k);
      case srplan::kWindowGood: break;
    }
    steps[i] = srplan::plan_audio_step(p.window, p.shift, step, c, k ? samples + sample_off[i] : nullptr, k, finishing);
    row_off[i + 1] = row_off[i] + steps[i].rows;
    rows_in[i] = steps[i].rows;
  }
  int rc = refuse_ids(named, ids, "push entry", "push");
  if (rc) return rc;
  // (uploaded asynchronously: alive until push_tail has synchronised)
  std::vector<int16_t> pieces;
  std::vector<StreamFrontendJob> jobs;
  rc = push_tail(s, slots, rows_in, finishing, out_feats, cap_rows, out_frame_off, [&](const PipelinePush& pp, PushFeed* fd) -> int {
    int rc = check_model(m);
    if (rc) return rc;
    fd->in_off = row_off.data();
    // the pieces (prev | tail | new samples) and the kernel's jobs: every utterance that gains a static or a row
    uint64_t stage_rows = 0;
    for (uint32_t i = 0; i < n; i++) {
      const srplan::AudioStep& st = steps[i];
      if (!st.new_statics && !st.rows) continue;
      const srplan::AudioCarry& c = au.carry[slots[i]];
      const uint64_t k = sample_off ? sample_off[i + 1] - sample_off[i] : 0;
      StreamFrontendJob j{};
      j.slot = slots[i]; j.S = (uint32_t)c.statics; j.k = (uint32_t)st.new_statics;
      j.T = finishing ? (uint32_t)st.next.statics : kStreamFrontendOpen;
      j.row0 = (uint32_t)st.row0; j.rows = (uint32_t)st.rows; j.warp = au.warp[slots[i]];
      j.sample0 = pieces.size(); j.stage0 = stage_rows; j.out0 = row_off[i];
      pieces.resize(pieces.size() + 1 + st.n_buf);
      srplan::audio_fill(c, st, k ? samples + sample_off[i] : nullptr, k, pieces.data() + j.sample0);
      stage_rows += H + st.new_statics;
      jobs.push_back(j);
    }
    if (jobs.empty()) return SR_OK;
    HIP_TRY(au.samples.ensure(pieces.size()));
    HIP_TRY(au.stage.ensure((size_t)stage_rows * nf));
    HIP_TRY(au.jobs.ensure(jobs.size()));
    if (pp.active) HIP_TRY(s->pipe.in.ensure((size_t)row_off[n] * fe->model->dim));
    else HIP_TRY(s->feats.ensure((size_t)pp.out_off[n] * m->dim));
    HIP_TRY(hipMemcpyAsync(au.samples.p, pieces.data(), sizeof(int16_t) * pieces.size(), hipMemcpyHostToDevice, m->s_gmm));
    HIP_TRY(hipMemcpyAsync(au.jobs.p, jobs.data(), sizeof(StreamFrontendJob) * jobs.size(), hipMemcpyHostToDevice, m->s_gmm));
    StreamFrontendArgs a{};
    MfccArgs& f = a.mfcc;
    f.samples = au.samples.p; f.span_frames = fe->span_frames;
    f.window = p.window; f.shift = p.shift; f.n_fft = p.n_fft; f.n_mel = p.n_mel; f.n_cepstra = p.n_cepstra;
    f.preemphasis = p.preemphasis; f.energy_floor = p.energy_floor;
    f.win = fe->win.p; f.twiddle = fe->twiddle.p; f.mel_first = fe->mel_first.p; f.mel_count = fe->mel_count.p; f.mel_off = fe->mel_off.p;
    f.mel_w = fe->mel_w.p; f.dct = fe->dct.p;
    f.warp_first = fe->warp_first.p; f.warp_count = fe->warp_count.p; f.warp_off = fe->warp_off.p; f.warp_w = fe->warp_w.p;  // (the jobs' warps)
    a.jobs = au.jobs.p;
    a.n_static = nf; a.n_first = fe->post.n_first; a.n_second = fe->post.n_second; a.step = step;
    a.mean = fe->normalise ? fe->mean.p : nullptr; a.stddev = fe->normalise ? fe->stddev.p : nullptr;
    a.energy_max_norm = fe->post.energy_max_norm != 0;
    a.state = au.state.p; a.stage = au.stage.p; a.out = pp.active ? s->pipe.in.p : s->feats.p;
    EventPair ep{};
    if ((rc = prof_begin(m, m->s_gmm, 1, &ep))) return rc;
    HIP_TRY(launch_stream_frontend(a, (uint32_t)jobs.size(), m->s_gmm));
    if ((rc = prof_end(m, m->s_gmm, &ep))) return rc;
    fd->queued = true;
    return SR_OK;
  });
  if (rc) return rc;
  for (uint32_t i = 0; i < n; i++) {
    au.carry[slots[i]] = std::move(steps[i].next);
    au.kind[slots[i]] = finishing ? kStreamAudioFinished : kStreamAudio;
  }
  return SR_OK;
}

// ---- the lifecycle --------------------------------------------------------------------------------------------------------------------
// what both _open calls ask of their sizes and of the scoring kernel, after their own net and params
int open_check(int gmm_kernel, uint32_t max_streams, uint64_t max_frames) {
  if (gmm_kernel < SR_GMM_MFMA || gmm_kernel > SR_GMM_DEFAULT) return fail(SR_EINVAL, "unknown gmm_kernel %d", gmm_kernel);
  if (max_streams == 0) return fail(SR_EINVAL, "max_streams must be at least 1");
  if (max_frames == 0) return fail(SR_EINVAL, "max_frames must be at least 1");
  return SR_OK;
}
void open_set(StreamSet* s, sr_model* m, uint32_t max_streams, uint64_t max_frames) {
  s->model = m;
  s->slots = StreamSlots(max_streams, max_frames);
  s->commit_fresh.assign(max_streams, 1);
  s->base.assign(max_streams, 0);
  s->audio.open(max_streams);
  s->pipe.open(max_streams);
}
// a fresh utterance in the first free slot: the first push starts from the initial state (the search kernels), the first stable call
// from commit point 0 (the start entry), with nothing trimmed
int begin_set(StreamSet* s, uint32_t* id, uint32_t* slot) {
  if (!s || !id) return fail(SR_EINVAL, "null argument");
  const int64_t at = s->slots.begin();
  if (at < 0) return fail(SR_ELIMIT, "all %u streams are open", s->slots.max_streams);
  *slot = (uint32_t)at;
  *id = s->slots.id[at];
  s->commit_fresh[at] = 1;
  s->base[at] = 0;
  s->audio.begin(*slot);
  s->pipe.begin(*slot);
  return SR_OK;
}
// the checks of an _end call behind its arguments: the id's slot; rows received and not yet searched keep a row id open
int end_check(const StreamSet* s, uint32_t id, const char* finish_audio, uint32_t* slot) {
  int rc = slot_of(s, id, slot);
  if (rc) return rc;
  if (s->audio.kind[*slot] == kStreamAudio) return fail(SR_EINVAL, "stream id %u is fed as audio and not finished (%s)", id, finish_audio);
  const srplan::PipelineCarry& c = s->pipe.carry[*slot];
  if (c.received > c.searched)
    return fail(SR_EINVAL, "stream id %u has %llu rows that wait for their right context: finish it first (sr_stream_push_rows)", id,
                (unsigned long long)(c.received - c.searched));
  return check_model(s->model);
}
void close_slot(StreamSet* s, uint32_t slot) {
  s->slots.open[slot] = 0;
  s->audio.end(slot);
}
int destroy_set(StreamSet* s) {
  if (!s) return SR_OK;
  if (s->model) { (void)hipSetDevice(s->model->device); (void)hipDeviceSynchronize(); }
  delete s;
  return SR_OK;
}

// ---- the pinned job block of the stable and trim calls ----------------------------------------------------------------------------------
// One call over n open utterances of a set (Job: StableJob, or BigramStableJob), one workgroup per utterance, through the set's pinned
// block (srplan::block_layout): Job[n] in, StableResult[n] and the items out, which the kernel writes straight into it.  The caller
// supplies make_job(i, slot, frames before, &job) -> rc; launch(jobs, results, items, frames, stream) -> rc over the block's three
// parts; accept(i, job, result) -> whether the result passes the call's checks, taking over what the call takes over from a good one;
// and what a bad one says.  Every good result is accepted -- the kernel left its commit point in commit[slot] -- before the first bad one
// is reported, and an id whose result is bad changes nothing.  *out: the jobs and, in the block, their results (n == 0: neither).
template <class Job>
struct BlockRun {
  std::vector<Job> jobs;
  const StableResult* res = nullptr;
};
template <class Job, class MakeJob, class Launch, class Accept>
int run_block(StreamSet* s, uint32_t n, const uint32_t* ids, bool null_argument, size_t frame_bytes, const char* corrupt, MakeJob make_job,
              Launch launch, Accept accept, BlockRun<Job>* out) {
  if (!s) return fail(SR_EINVAL, "null stream set");
  if (null_argument) return fail(SR_EINVAL, "null argument");
  sr_model* m = s->model;
  int rc = check_model(m);
  if (rc) return rc;
  const StreamSlots& sl = s->slots;
  std::vector<Job>& jobs = out->jobs;
  jobs.resize(n);
  // (the slots go straight into the jobs' slot fields, which spares an array; make_job then writes the whole record, its slot included)
  static_assert(std::is_same<decltype(Job::slot), uint32_t>::value, "resolve_ids stores 32-bit slots");
  const srplan::IdResolution named = srplan::resolve_ids(sl, n, ids, n ? &jobs[0].slot : nullptr, sizeof(Job));
  uint64_t F = 0;
  for (uint32_t i = 0; i < named.entry; i++) {
    const uint32_t slot = jobs[i].slot;
    if ((rc = make_job(i, slot, F, &jobs[i]))) return rc;
    F += sl.frames[slot];
  }
  if ((rc = refuse_ids(named, ids, "entry", "call"))) return rc;
  if (n == 0) return SR_OK;
  HIP_TRY(s->commit.ensure(sl.max_streams));
  const srplan::BlockLayout at = srplan::block_layout(sizeof(Job), sizeof(StableResult), frame_bytes, n, F);
  if (at.need > s->stable_block.n) HIP_TRY(s->stable_block.ensure(srplan::block_grown(at.need, s->stable_block.n)));
  unsigned char* blk = s->stable_block.p;
  memcpy(blk, jobs.data(), sizeof(Job) * n);
  StableResult* res = reinterpret_cast<StableResult*>(blk + at.res_at);
  if ((rc = launch(reinterpret_cast<const Job*>(blk), res, blk + at.items_at, F, m->s_gmm))) return rc;
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  uint32_t bad = 0xFFFFFFFFu;
  for (uint32_t i = 0; i < n; i++) {
    if (accept(i, jobs[i], res[i])) s->commit_fresh[jobs[i].slot] = 0;
    else if (bad == 0xFFFFFFFFu) bad = i;
  }
  if (bad != 0xFFFFFFFFu) return fail(SR_ECORRUPT, "stream %u: %s", ids[bad], corrupt);
  out->res = res;
  return SR_OK;
}
// A stable call behind run_block: the items of utterance i (lead(slot) of them precede the kernel's: the archive of a trimmed zerogram
// id) start at out_off[i]; the caller's arrays must hold them all (`holds`: the middle of the message); copy_out(i, job, result,
// out_off[i]) hands them over (it may restate out_commit[i]).
template <class Job, class Lead, class CopyOut>
int stable_out(const BlockRun<Job>& run, uint32_t n, uint64_t cap, const char* holds, uint64_t* out_off, uint32_t* out_commit, Lead lead,
               CopyOut copy_out) {
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; i++) { out_off[i] = total; total += lead(run.jobs[i].slot) + run.res[i].count; }
  out_off[n] = total;
  if (total > cap) return fail(SR_EINVAL, "%llu stable %s %llu", (unsigned long long)total, holds, (unsigned long long)cap);
  for (uint32_t i = 0; i < n; i++) {
    out_commit[i] = run.res[i].commit;
    copy_out(i, run.jobs[i], run.res[i], out_off[i]);
  }
  return SR_OK;
}
// a stable result that passes: a commit point and a word count within the frames searched
template <class Job>
bool stable_good(uint32_t, const Job& j, const StableResult& r) { return !(r.flags || r.count > j.t || r.commit > j.t); }
}  // namespace

// ---- streaming recognition (sr_stream_*): decode_stream_kernel over per-slot state in device memory ---------------------------

int sr_stream_open(sr_model* m, sr_lexicon* l, const sr_search_params* p, uint32_t max_streams, uint64_t max_frames, sr_stream** out) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  int rc = check_model(m);
  if (rc) return rc;
  if (!l || l->model != m) return fail(SR_EINVAL, "lexicon does not belong to this model");
  if (!p) return fail(SR_EINVAL, "null search params");
  if (p->flags != 0) return fail(SR_EINVAL, "sr_search_params.flags must be 0 for streaming (got 0x%x)", (unsigned)p->flags);
  if ((rc = open_check(p->gmm_kernel, max_streams, max_frames))) return rc;
  if (max_frames > 65535) return fail(SR_ELIMIT, "max_frames %llu: back pointers are 16 bit like the reference's Book::bkp (max 65535)", (unsigned long long)max_frames);
  if (l->net.n_slots > decode_big_max_slots()) return fail(SR_ELIMIT, "%u trellis positions exceed the stream search's limit of %u", l->net.n_slots, decode_big_max_slots());
  sr_stream* s = new sr_stream();
  std::unique_ptr<sr_stream, int (*)(sr_stream*)> own(s, sr_stream_destroy);
  open_set(s, m, max_streams, max_frames);
  s->lex = l; s->params = *p;
  s->archive.assign(max_streams, std::vector<uint32_t>());
  const size_t S = max_streams;
  HIP_TRY(s->ws.ensure(S * decode_big_workspace(l->net.n_slots)));
  HIP_TRY(s->state.ensure(S));
  HIP_TRY(s->tb_score.ensure(S * (max_frames + 1)));
  HIP_TRY(s->tb_word.ensure(S * (max_frames + 1)));
  HIP_TRY(s->tb_bkp.ensure(S * (max_frames + 1)));
  HIP_TRY(s->words.ensure(S * max_frames));
  *out = own.release();
  return SR_OK;
  });
}

int sr_stream_begin(sr_stream* s, uint32_t* id) {
  return guarded(__func__, [&]() -> int {
  uint32_t slot = 0;
  const int rc = begin_set(s, id, &slot);
  if (rc) return rc;
  s->archive[slot].clear();
  return SR_OK;
  });
}

int sr_stream_push(sr_stream* s, uint32_t n, const uint32_t* ids, const float* feats, const uint64_t* frame_off) {
  return guarded(__func__, [&]() -> int { return push_rows(s, n, ids, feats, frame_off, false, nullptr, 0, nullptr); });
}
int sr_stream_push_rows(sr_stream* s, uint32_t n, const uint32_t* ids, const float* feats, const uint64_t* frame_off, int finish,
                        float* out_feats, uint64_t cap_rows, uint64_t* out_frame_off) {
  return guarded(__func__, [&]() -> int { return push_rows(s, n, ids, feats, frame_off, finish != 0, out_feats, cap_rows, out_frame_off); });
}
int sr_stream_set_projection(sr_stream* s, uint32_t in_dim, uint32_t context, const double* M) {
  return guarded(__func__, [&]() -> int { return set_projection(s, in_dim, context, M); });
}
int sr_stream_set_transform(sr_stream* s, uint32_t id, const double* W) {
  return guarded(__func__, [&]() -> int { return set_transform(s, id, W); });
}

int sr_stream_set_frontend(sr_stream* s, sr_frontend* fe) {
  return guarded(__func__, [&]() -> int { return set_frontend(s, fe); });
}
int sr_stream_set_warp(sr_stream* s, uint32_t id, uint32_t warp) {
  return guarded(__func__, [&]() -> int { return set_warp(s, id, warp); });
}
int sr_stream_push_audio(sr_stream* s, uint32_t n, const uint32_t* ids, const int16_t* samples, const uint64_t* sample_off, float* out_feats,
                         uint64_t cap_rows, uint64_t* out_frame_off) {
  return guarded(__func__, [&]() -> int { return push_audio(s, n, ids, samples, sample_off, false, out_feats, cap_rows, out_frame_off); });
}
int sr_stream_finish_audio(sr_stream* s, uint32_t n, const uint32_t* ids, float* out_feats, uint64_t cap_rows, uint64_t* out_frame_off) {
  return guarded(__func__, [&]() -> int { return push_audio(s, n, ids, nullptr, nullptr, true, out_feats, cap_rows, out_frame_off); });
}

int sr_stream_partial(sr_stream* s, uint32_t id, uint32_t* out_words, uint32_t cap, uint32_t* count, uint64_t* frames) {
  return guarded(__func__, [&]() -> int {
  if (!s || !count || (!out_words && cap)) return fail(SR_EINVAL, "null argument");
  uint32_t slot = 0;
  int rc = slot_of(s, id, &slot);
  if (rc || (rc = check_model(s->model))) return rc;
  if (frames) *frames = s->base[slot] + s->slots.frames[slot];
  return stream_words(s, slot, id, out_words, cap, count);
  });
}

int sr_stream_end(sr_stream* s, uint32_t id, uint32_t* out_words, uint32_t cap, uint32_t* count, double* tb_score, uint16_t* tb_word,
                  uint16_t* tb_bkp) {
  return guarded(__func__, [&]() -> int {
  if (!s || !count || (!out_words && cap)) return fail(SR_EINVAL, "null argument");
  uint32_t slot = 0;
  int rc = end_check(s, id, "sr_stream_finish_audio", &slot);
  if (rc) return rc;
  if (s->base[slot] && (tb_score || tb_word || tb_bkp))
    return fail(SR_EINVAL, "stream id %u has been trimmed: the traceback entries of its first %llu frames are gone (pass NULL arrays)", id,
                (unsigned long long)s->base[slot]);
  rc = stream_words(s, slot, id, out_words, cap, count);
  if (rc == SR_EINVAL) return rc;  // too small a buffer: the utterance stays open
  const uint64_t T = s->slots.frames[slot];
  if (rc == SR_OK && T == 0) {  // traceback[0] of the empty utterance (Recognizer.cpp:118-120)
    if (tb_score) tb_score[0] = 0.0;
    if (tb_word) tb_word[0] = 0;
    if (tb_bkp) tb_bkp[0] = 0;
  } else if (rc == SR_OK) {
    const size_t b = (size_t)slot * (s->slots.max_frames + 1);
    if (tb_score) HIP_TRY(hipMemcpy(tb_score, s->tb_score.p + b, sizeof(double) * (T + 1), hipMemcpyDeviceToHost));
    if (tb_word) HIP_TRY(hipMemcpy(tb_word, s->tb_word.p + b, sizeof(uint16_t) * (T + 1), hipMemcpyDeviceToHost));
    if (tb_bkp) HIP_TRY(hipMemcpy(tb_bkp, s->tb_bkp.p + b, sizeof(uint16_t) * (T + 1), hipMemcpyDeviceToHost));
  }
  close_slot(s, slot);
  std::vector<uint32_t>().swap(s->archive[slot]);
  return rc;
  });
}

// The stable prefix: one launch of stream_commit_kernel.  The block's items are the words (4 bytes a frame), utterance i's at
// jobs[i].word_off.
int sr_stream_stable(sr_stream* s, uint32_t n, const uint32_t* ids, uint32_t* out_words, uint64_t cap, uint64_t* out_word_off,
                     uint32_t* out_commit, uint32_t* out_silence) {
  return guarded(__func__, [&]() -> int {
  const uint32_t* words = nullptr;
  BlockRun<StableJob> run;
  int rc = run_block(
      s, n, ids, !out_word_off || (n && (!ids || !out_commit)) || (!out_words && cap), sizeof(uint32_t),
      "the traceback does not walk back from the commit point to frame 0 (Recognizer.cpp:222-231)",
      [&](uint32_t, uint32_t slot, uint64_t off, StableJob* job) -> int {
        if (s->base[slot] + s->slots.frames[slot] > 0xFFFFFFFFull)  // (out_commit = base + c, c <= the window's frames)
          return fail(SR_ELIMIT, "stream id %u: a commit frame past 2^32 - 1 does not fit out_commit", s->slots.id[slot]);
        *job = StableJob{slot, (uint32_t)s->slots.frames[slot], s->commit_fresh[slot], 0u, off};
        return SR_OK;
      },
      [&](const StableJob* jobs, StableResult* res, unsigned char* items, uint64_t, hipStream_t stream) -> int {
        const StreamSlots& sl = s->slots;
        const sr_lexicon* l = s->lex;
        HIP_TRY(s->stable_words.ensure((size_t)sl.max_streams * sl.max_frames));
        StableArgs a{};
        a.net = l->net;
        a.jobs = jobs;
        a.ws = s->ws.p; a.ws_stride = decode_big_workspace(l->net.n_slots);
        a.tb_word = s->tb_word.p; a.tb_bkp = s->tb_bkp.p; a.tb_stride = sl.max_frames + 1;
        a.commit = s->commit.p; a.words = s->stable_words.p; a.words_stride = sl.max_frames;
        a.out_res = res; a.out_words = reinterpret_cast<uint32_t*>(items);
        words = a.out_words;
        HIP_TRY(launch_stream_commit(a, n, stream));
        return SR_OK;
      },
      stable_good<StableJob>, &run);
  if (rc) return rc;
  return stable_out(
      run, n, cap, "words, out_words holds", out_word_off, out_commit, [&](uint32_t slot) -> uint64_t { return s->archive[slot].size(); },
      [&](uint32_t i, const StableJob& job, const StableResult& r, uint64_t at) {
        // a trimmed utterance: the archive's words lead (every commit point lies on the chain through the last one trimmed at),
        // and the commit frame counts from the utterance's start
        const std::vector<uint32_t>& arch = s->archive[job.slot];
        if (!arch.empty()) memcpy(out_words + at, arch.data(), sizeof(uint32_t) * arch.size());
        if (r.count) memcpy(out_words + at + arch.size(), words + job.word_off, sizeof(uint32_t) * r.count);
        out_commit[i] = (uint32_t)(s->base[job.slot] + r.commit);
        if (out_silence) out_silence[i] = r.silence;
      });
  });
}

// sr_stream_trim (include/srgpu.h has the definition): one launch of stream_trim_kernel over the block of a stable call, the committed
// words its items.  Everything is checked before the launch; an id whose result is flagged has written nothing on the device.
int sr_stream_trim(sr_stream* s, uint32_t n, const uint32_t* ids, uint32_t* out_dropped) {
  return guarded(__func__, [&]() -> int {
  const uint32_t* words = nullptr;
  BlockRun<StableJob> run;
  int rc = run_block(
      s, n, ids, n && !ids, sizeof(uint32_t),
      "the traceback does not walk back from the commit point to frame 0, or an alive hypothesis starts below it",
      [&](uint32_t, uint32_t slot, uint64_t off, StableJob* job) -> int {
        *job = StableJob{slot, (uint32_t)s->slots.frames[slot], s->commit_fresh[slot], 0u, off};
        return SR_OK;
      },
      [&](const StableJob* jobs, StableResult* res, unsigned char* items, uint64_t, hipStream_t stream) -> int {
        const StreamSlots& sl = s->slots;
        const sr_lexicon* l = s->lex;
        HIP_TRY(s->stable_words.ensure((size_t)sl.max_streams * sl.max_frames));
        TrimArgs a{};
        a.net = l->net;
        a.jobs = jobs;
        a.ws = s->ws.p; a.ws_stride = decode_big_workspace(l->net.n_slots); a.state = s->state.p;
        a.tb_score = s->tb_score.p; a.tb_word = s->tb_word.p; a.tb_bkp = s->tb_bkp.p; a.tb_stride = sl.max_frames + 1;
        a.commit = s->commit.p; a.walk_words = s->stable_words.p; a.words = s->words.p; a.words_stride = sl.max_frames;
        a.out_res = res; a.out_words = reinterpret_cast<uint32_t*>(items);
        words = a.out_words;
        HIP_TRY(launch_stream_trim(a, n, stream));
        return SR_OK;
      },
      [&](uint32_t i, const StableJob& j, const StableResult& r) -> bool {
        // a hypothesis entered at frame t carries bkp = t - 1: the commit point is below t and the window keeps a frame
        if (r.flags || r.count > r.commit || (j.t ? r.commit >= j.t : r.commit != 0)) return false;
        s->archive[j.slot].insert(s->archive[j.slot].end(), words + j.word_off, words + j.word_off + r.count);
        s->base[j.slot] += r.commit;
        s->slots.frames[j.slot] -= r.commit;
        if (out_dropped) out_dropped[i] = r.commit;
        return true;
      },
      &run);
  return rc;
  });
}

// test hook: the nearest-common-ancestor fold of commit_point.h alone, on forests the caller supplies
int sr_commit_points(sr_model* m, uint32_t n_sets, const uint64_t* node_off, const uint32_t* parent, const uint64_t* set_off,
                     const uint32_t* set, const uint32_t* floor, uint32_t* out) {
  return guarded(__func__, [&]() -> int {
  int rc = check_model(m);
  if (rc) return rc;
  if (n_sets == 0) return SR_OK;
  if (!node_off || !parent || !set_off || !set || !floor || !out) return fail(SR_EINVAL, "null argument");
  if (node_off[0] != 0 || set_off[0] != 0) return fail(SR_EINVAL, "node_off[0] and set_off[0] must be 0");
  for (uint32_t i = 0; i < n_sets; i++) {
    if (node_off[i + 1] <= node_off[i]) return fail(SR_EINVAL, "set %u: a tree has at least its root", i);
    if (set_off[i + 1] <= set_off[i]) return fail(SR_EINVAL, "set %u is empty", i);
    const uint64_t nn = node_off[i + 1] - node_off[i];
    if (nn >= 0xFFFFFFFEull) return fail(SR_ELIMIT, "set %u: %llu nodes, node indices are 32 bit", i, (unsigned long long)nn);
    const uint32_t* par = parent + node_off[i];
    if (par[0] != 0) return fail(SR_EINVAL, "set %u: parent[0] must be 0", i);
    for (uint64_t j = 1; j < nn; j++)
      if (par[j] >= j) return fail(SR_EINVAL, "set %u: parent[%llu] = %u is not below its child", i, (unsigned long long)j, par[j]);
    for (uint64_t j = set_off[i]; j < set_off[i + 1]; j++)
      if (set[j] >= nn) return fail(SR_EINVAL, "set %u: node %u out of range (%llu nodes)", i, set[j], (unsigned long long)nn);
    if (floor[i] >= nn) return fail(SR_EINVAL, "set %u: floor %u out of range (%llu nodes)", i, floor[i], (unsigned long long)nn);
  }
  DevBuf<uint64_t> d_node_off, d_set_off;
  DevBuf<uint32_t> d_parent, d_set, d_floor, d_out;
  HIP_TRY(d_node_off.upload(node_off, (size_t)n_sets + 1));
  HIP_TRY(d_set_off.upload(set_off, (size_t)n_sets + 1));
  HIP_TRY(d_parent.upload(parent, node_off[n_sets]));
  HIP_TRY(d_set.upload(set, set_off[n_sets]));
  HIP_TRY(d_floor.upload(floor, n_sets));
  HIP_TRY(d_out.ensure(n_sets));
  CommitPointsArgs a{d_node_off.p, d_parent.p, d_set_off.p, d_set.p, d_floor.p, d_out.p};
  HIP_TRY(launch_commit_points(a, n_sets, m->s_gmm));
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  std::vector<uint32_t> got(n_sets);
  HIP_TRY(hipMemcpy(got.data(), d_out.p, sizeof(uint32_t) * n_sets, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n_sets; i++)
    if (got[i] >= node_off[i + 1] - node_off[i]) return fail(SR_ECORRUPT, "set %u: the fold left the tree", i);
  memcpy(out, got.data(), sizeof(uint32_t) * n_sets);
  return SR_OK;
  });
}

int sr_stream_destroy(sr_stream* s) {
  return guarded(__func__, [&]() -> int { return destroy_set(s); });
}

// ---- streaming bigram-LM recognition (sr_bigram_stream_*): bigram_stream_kernel over per-slot state in device memory --------------

int sr_bigram_stream_open(sr_model* m, sr_bigram* b, const sr_bigram_params* p, uint32_t max_streams, uint64_t max_frames,
                          sr_bigram_stream** out) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  int rc = check_model(m);
  if (rc) return rc;
  if (!b || b->model != m) return fail(SR_EINVAL, "bigram search net does not belong to this model");
  if (!p) return fail(SR_EINVAL, "null bigram params");
  if (p->flags != 0) return fail(SR_EINVAL, "sr_bigram_params.flags must be 0 for streaming (got 0x%x)", (unsigned)p->flags);
  if (p->max_word_ends != 0)
    return fail(SR_EINVAL, "sr_bigram_params.max_word_ends must be 0 for streaming (got %u): the book grows with the utterance", p->max_word_ends);
  if ((rc = open_check(p->gmm_kernel, max_streams, max_frames))) return rc;
  if (max_frames > 0xFFFFFFFEull) return fail(SR_ELIMIT, "max_frames %llu: frame times are 32 bit", (unsigned long long)max_frames);
  sr_bigram_stream* s = new sr_bigram_stream();
  std::unique_ptr<sr_bigram_stream, int (*)(sr_bigram_stream*)> own(s, sr_bigram_stream_destroy);
  open_set(s, m, max_streams, max_frames);
  s->bigram = b; s->params = *p;
  s->host_state.assign(max_streams, BigramStreamState{}); s->failed.assign(max_streams, 0);
  const size_t S = max_streams, W = b->net.n_words;
  HIP_TRY(s->gs_ws.ensure(S * bigram_gs_ws_words(b->net.n_words, b->net.n_positions)));
  HIP_TRY(s->we_slot.ensure(S * 4 * W));
  HIP_TRY(s->we_bp.ensure(S * 4 * W));
  HIP_TRY(s->we_score.ensure(S * 4 * W));
  HIP_TRY(s->lsave.ensure(S * 2 * W));
  HIP_TRY(s->state.ensure(S));
  HIP_TRY(s->out_word.ensure(S * (max_frames + 1)));
  HIP_TRY(s->out_time.ensure(S * (max_frames + 1)));
  HIP_TRY(s->out_score.ensure(S * (max_frames + 1)));
  for (size_t i = 0; i < S; i++) s->book.emplace_back(new DevBuf<uint4>());
  *out = own.release();
  return SR_OK;
  });
}

int sr_bigram_stream_begin(sr_bigram_stream* s, uint32_t* id) {
  return guarded(__func__, [&]() -> int {
  uint32_t slot = 0;
  const int rc = begin_set(s, id, &slot);
  if (rc) return rc;
  s->host_state[slot] = BigramStreamState{};
  s->host_state[slot].n_book = 2;  // the two start entries the first push writes
  s->failed[slot] = 0;
  return SR_OK;
  });
}

int sr_bigram_stream_push(sr_bigram_stream* s, uint32_t n, const uint32_t* ids, const float* feats, const uint64_t* frame_off) {
  return guarded(__func__, [&]() -> int { return push_rows(s, n, ids, feats, frame_off, false, nullptr, 0, nullptr); });
}
int sr_bigram_stream_push_rows(sr_bigram_stream* s, uint32_t n, const uint32_t* ids, const float* feats, const uint64_t* frame_off, int finish,
                               float* out_feats, uint64_t cap_rows, uint64_t* out_frame_off) {
  return guarded(__func__, [&]() -> int { return push_rows(s, n, ids, feats, frame_off, finish != 0, out_feats, cap_rows, out_frame_off); });
}
int sr_bigram_stream_set_projection(sr_bigram_stream* s, uint32_t in_dim, uint32_t context, const double* M) {
  return guarded(__func__, [&]() -> int { return set_projection(s, in_dim, context, M); });
}
int sr_bigram_stream_set_transform(sr_bigram_stream* s, uint32_t id, const double* W) {
  return guarded(__func__, [&]() -> int { return set_transform(s, id, W); });
}

int sr_bigram_stream_set_frontend(sr_bigram_stream* s, sr_frontend* fe) {
  return guarded(__func__, [&]() -> int { return set_frontend(s, fe); });
}
int sr_bigram_stream_set_warp(sr_bigram_stream* s, uint32_t id, uint32_t warp) {
  return guarded(__func__, [&]() -> int { return set_warp(s, id, warp); });
}
int sr_bigram_stream_push_audio(sr_bigram_stream* s, uint32_t n, const uint32_t* ids, const int16_t* samples, const uint64_t* sample_off,
                                float* out_feats, uint64_t cap_rows, uint64_t* out_frame_off) {
  return guarded(__func__, [&]() -> int { return push_audio(s, n, ids, samples, sample_off, false, out_feats, cap_rows, out_frame_off); });
}
int sr_bigram_stream_finish_audio(sr_bigram_stream* s, uint32_t n, const uint32_t* ids, float* out_feats, uint64_t cap_rows,
                                  uint64_t* out_frame_off) {
  return guarded(__func__, [&]() -> int { return push_audio(s, n, ids, nullptr, nullptr, true, out_feats, cap_rows, out_frame_off); });
}

int sr_bigram_stream_partial(sr_bigram_stream* s, uint32_t id, uint32_t* out_word, float* out_score, uint32_t* out_time, uint32_t cap,
                             uint32_t* count, uint64_t* frames) {
  return guarded(__func__, [&]() -> int {
  if (!s || !count || ((!out_word || !out_score || !out_time) && cap)) return fail(SR_EINVAL, "null argument");
  uint32_t slot = 0;
  int rc = slot_of(s, id, &slot);
  if (rc || (rc = check_model(s->model))) return rc;
  if (frames) *frames = s->base[slot] + s->slots.frames[slot];
  return bigram_stream_items(s, slot, id, out_word, out_score, out_time, cap, count);
  });
}

int sr_bigram_stream_end(sr_bigram_stream* s, uint32_t id, uint32_t* out_word, float* out_score, uint32_t* out_time, uint32_t cap,
                         uint32_t* count) {
  return guarded(__func__, [&]() -> int {
  if (!s || !count || ((!out_word || !out_score || !out_time) && cap)) return fail(SR_EINVAL, "null argument");
  uint32_t slot = 0;
  int rc = end_check(s, id, "sr_bigram_stream_finish_audio", &slot);
  if (rc) return rc;
  rc = bigram_stream_items(s, slot, id, out_word, out_score, out_time, cap, count);
  if (rc == SR_EINVAL) return rc;  // too small a buffer: the utterance stays open
  close_slot(s, slot);
  return rc;
  });
}

// The stable prefix: one launch of bigram_stream_commit_kernel.  The block's items are three areas (word, score, time: 12 bytes a
// frame), utterance i's at jobs[i].item_off of each.
int sr_bigram_stream_stable(sr_bigram_stream* s, uint32_t n, const uint32_t* ids, uint32_t* out_word, float* out_score,
                            uint32_t* out_time, uint64_t cap, uint64_t* out_off, uint32_t* out_commit) {
  return guarded(__func__, [&]() -> int {
  BigramStableArgs a{};
  BlockRun<BigramStableJob> run;
  int rc = run_block(
      s, n, ids, !out_off || (n && (!ids || !out_commit)) || ((!out_word || !out_score || !out_time) && cap), 12,
      "the book walk from the commit entry does not end at its start entry",
      [&](uint32_t i, uint32_t slot, uint64_t off, BigramStableJob* job) -> int {
        if (s->failed[slot]) return fail(SR_EINTERNAL, "stream %u: a push overflowed its book", ids[i]);
        const uint64_t t = s->slots.frames[slot];
        *job = BigramStableJob{slot, (uint32_t)t, s->commit_fresh[slot], 0u, t ? s->book[slot]->p : nullptr, off};
        return SR_OK;
      },
      [&](const BigramStableJob* jobs, StableResult* res, unsigned char* items, uint64_t N, hipStream_t stream) -> int {
        const sr_bigram* b = s->bigram;
        a.n_words = b->net.n_words; a.silence = b->net.silence; a.n_positions = b->net.n_positions; a.slot_off = b->net.slot_off;
        a.gs_ws = s->gs_ws.p; a.gs_ws_words = bigram_gs_ws_words(b->net.n_words, b->net.n_positions);
        a.we_bp = s->we_bp.p; a.lsave = s->lsave.p; a.state = s->state.p;
        a.jobs = jobs;
        a.commit = s->commit.p;
        a.out_res = res;
        a.out_word = reinterpret_cast<uint32_t*>(items);
        a.out_score = reinterpret_cast<float*>(items + 4 * N);
        a.out_time = reinterpret_cast<uint32_t*>(items + 8 * N);
        HIP_TRY(launch_bigram_stream_commit(a, n, stream));
        return SR_OK;
      },
      stable_good<BigramStableJob>, &run);
  if (rc) return rc;
  return stable_out(
      run, n, cap, "items, the output arrays hold", out_off, out_commit, [](uint32_t) -> uint64_t { return 0; },
      [&](uint32_t, const BigramStableJob& job, const StableResult& r, uint64_t at) {
        if (!r.count) return;
        memcpy(out_word + at, a.out_word + job.item_off, sizeof(uint32_t) * r.count);
        memcpy(out_score + at, a.out_score + job.item_off, sizeof(float) * r.count);
        memcpy(out_time + at, a.out_time + job.item_off, sizeof(uint32_t) * r.count);
      });
  });
}

int sr_bigram_stream_destroy(sr_bigram_stream* s) {
  return guarded(__func__, [&]() -> int { return destroy_set(s); });
}
