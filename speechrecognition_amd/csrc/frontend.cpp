// frontend.cpp -- the host side of the audio front end (include/srgpu.h: sr_frontend_*, sr_corpus_from_audio, sr_corpus_from_cepstra,
// sr_mfcc_corpus, sr_corpus_download; with warps: sr_frontend_create_warped, sr_corpus_from_audio_warped, sr_vtln_costs_corpus): the
// argument checks, the MFCC stage's tables -- computed in double, stored as float; the filters' builder is vtln_tables.h -- and the
// entry points.  The kernels are frontend.hip.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "handles.h"

using srhost::fail;
using srhost::guarded;

namespace {

constexpr uint32_t kSpanFrames = 16;  // most frames a workgroup of mfcc_kernel covers

struct MfccTables {
  std::vector<float> win, dct;
  std::vector<float2> twiddle;
  srplan::MelTables mel;   // the unwarped filters
  srplan::MelTables warp;  // a warped front end's: one CSR over (warp, filter)
};

int check_mfcc(const sr_mfcc_params& p) {
  if (p.shift == 0) return fail(SR_EINVAL, "mfcc: shift is 0");
  if (p.window < 2) return fail(SR_EINVAL, "mfcc: window must be at least 2 samples");
  if (p.n_fft < 64 || p.n_fft > 2048 || (p.n_fft & (p.n_fft - 1)))
    return fail(SR_ELIMIT, "mfcc: n_fft %u is not a power of two in 64 .. 2048", p.n_fft);
  if (p.window > p.n_fft) return fail(SR_ELIMIT, "mfcc: window %u exceeds n_fft %u", p.window, p.n_fft);
  if (p.n_mel > 64) return fail(SR_ELIMIT, "mfcc: %u filters; a wave sums one per lane (at most 64)", p.n_mel);
  if (p.n_cepstra == 0 || p.n_cepstra > p.n_mel) return fail(SR_EINVAL, "mfcc: n_cepstra must be 1 .. n_mel");
  if (!(p.sample_rate > 0.0) || !std::isfinite(p.sample_rate)) return fail(SR_EINVAL, "mfcc: sample_rate must be positive and finite");
  if (!(p.f_low >= 0.0)) return fail(SR_EINVAL, "mfcc: f_low must be >= 0");
  if (!(p.f_high <= 0.5 * p.sample_rate)) return fail(SR_EINVAL, "mfcc: f_high must be <= sample_rate / 2");
  if (!(p.f_low < p.f_high)) return fail(SR_EINVAL, "mfcc: f_low must be below f_high");
  if (!(p.energy_floor > 0.0f) || !std::isfinite(p.energy_floor)) return fail(SR_EINVAL, "mfcc: energy_floor must be positive and finite");
  if (!std::isfinite(p.preemphasis)) return fail(SR_EINVAL, "mfcc: preemphasis is not finite");
  if (p.flags != 0) return fail(SR_EINVAL, "mfcc: flags must be 0");
  return SR_OK;
}

// the tables of include/srgpu.h's definition (the filters: vtln_tables.h); SR_EINVAL for a filter without a bin of positive weight.
// vtln != NULL: the warps' filters too.  Window, twiddles and DCT are shared by all warps.
int build_tables(const sr_mfcc_params& p, const sr_vtln_params* vtln, MfccTables* t) {
  const double pi = 3.14159265358979323846;
  const uint32_t N = p.n_fft;
  t->win.resize(p.window);
  for (uint32_t i = 0; i < p.window; i++) t->win[i] = (float)(0.54 - 0.46 * std::cos(2.0 * pi * i / (p.window - 1)));
  t->twiddle.resize(N);
  for (uint32_t n = 0; n < N; n++) {
    const double ang = 2.0 * pi * n / N;
    t->twiddle[n] = make_float2((float)std::cos(ang), (float)-std::sin(ang));
  }
  double l = 0.0, r = 0.0;
  int bad = srplan::append_mel_filters(p.sample_rate, N, p.n_mel, p.f_low, p.f_high, 1.0, 0.5, &t->mel, &l, &r);
  if (bad >= 0) return fail(SR_EINVAL, "mfcc: filter %d (%.1f .. %.1f Hz) has no bin of positive weight", bad, l, r);
  for (uint32_t a = 0; vtln && a < vtln->n_warps; a++) {
    bad = srplan::append_mel_filters(p.sample_rate, N, p.n_mel, p.f_low, p.f_high, vtln->alpha[a], vtln->break_frac, &t->warp, &l, &r);
    if (bad >= 0)
      return fail(SR_EINVAL, "vtln: warp %u (alpha %g), filter %d (%.1f .. %.1f Hz) has no bin of positive weight", a, vtln->alpha[a], bad, l, r);
  }
  t->dct.resize((size_t)p.n_cepstra * p.n_mel);
  const double scale = std::sqrt(2.0 / p.n_mel);
  for (uint32_t i = 0; i < p.n_cepstra; i++)
    for (uint32_t m = 0; m < p.n_mel; m++) t->dct[(size_t)i * p.n_mel + m] = (float)(scale * std::cos(pi * i * (m + 0.5) / p.n_mel));
  return SR_OK;
}

// sr_profile_*: the kernels' event pairs, counted with the search's (kind 1) like the other corpus transforms'
int prof_begin(sr_model* m, EventPair* ep) {
  if (!m->profiling) return SR_OK;
  ep->kind = 1;
  HIP_TRY(hipEventCreate(&ep->a));
  HIP_TRY(hipEventCreate(&ep->b));
  HIP_TRY(hipEventRecord(ep->a, m->s_gmm));
  return SR_OK;
}
int prof_end(sr_model* m, EventPair* ep) {
  if (!m->profiling) return SR_OK;
  HIP_TRY(hipEventRecord(ep->b, m->s_gmm));
  m->events.push_back(*ep);
  return SR_OK;
}

uint64_t frames_of(const sr_mfcc_params& p, uint64_t n) { return n < p.window ? 0 : 1 + (n - p.window) / p.shift; }

int check_frontend(const sr_frontend* fe) {
  if (!fe || !fe->model) return fail(SR_EINVAL, "null front end handle");
  HIP_TRY(hipSetDevice(fe->model->device));
  return SR_OK;
}

// offsets that start at 0 and do not fall; frames: no utterance beyond what a corpus takes
int check_offsets(const uint64_t* off, uint32_t n_utts, const char* name) {
  if (!off) return fail(SR_EINVAL, "%s is null", name);
  if (off[0] != 0) return fail(SR_EINVAL, "%s[0] must be 0", name);
  for (uint32_t u = 0; u < n_utts; u++)
    if (off[u + 1] < off[u]) return fail(SR_EINVAL, "%s must be non-decreasing (utterance %u)", name, u);
  return SR_OK;
}
int check_frame_counts(const uint64_t* frame_off, uint32_t n_utts) {
  for (uint32_t u = 0; u < n_utts; u++)
    if (frame_off[u + 1] - frame_off[u] > 65535)
      return fail(SR_ELIMIT, "utterance %u has %llu frames; back pointers are 16 bit like the reference's Book::bkp (max 65535)", u,
                  (unsigned long long)(frame_off[u + 1] - frame_off[u]));
  return SR_OK;
}

// the checks of a call that takes samples, before any launch; frame_off [n_utts + 1] filled
int check_audio(const sr_frontend* fe, const int16_t* samples, const uint64_t* sample_off, uint32_t n_utts, std::vector<uint64_t>* frame_off) {
  if (!fe->has_mfcc) return fail(SR_EINVAL, "this front end was made without an MFCC stage: it takes cepstra only");
  int rc = check_offsets(sample_off, n_utts, "sample_off");
  if (rc) return rc;
  if (sample_off[n_utts] > 0 && !samples) return fail(SR_EINVAL, "samples is null");
  frame_off->assign((size_t)n_utts + 1, 0);
  for (uint32_t u = 0; u < n_utts; u++) (*frame_off)[u + 1] = (*frame_off)[u] + frames_of(fe->mfcc, sample_off[u + 1] - sample_off[u]);
  return check_frame_counts(frame_off->data(), n_utts);
}

// samples -> static cepstra on the device (run_mfcc), cep [frames x n_cepstra]; queued on the model's scoring stream, not waited for.
// `keep` holds the launch's inputs until the caller has synchronised
struct AudioInputs {
  DevBuf<int16_t> samples;
  DevBuf<uint64_t> sample_off, frame_off;
  DevBuf<uint2> spans;
  DevBuf<uint32_t> utt_warp;
  srgpu::MfccArgs args{};  // everything but `out`, the warps and their filters
};
// the samples, offsets and spans of a batch on the device, and the launch's arguments as far as they do not depend on the warps
int upload_audio(sr_frontend* fe, const int16_t* samples, const uint64_t* sample_off, uint32_t n_utts, const std::vector<uint64_t>& frame_off,
                 AudioInputs* keep) {
  const sr_mfcc_params& p = fe->mfcc;
  std::vector<uint2> spans;
  for (uint32_t u = 0; u < n_utts; u++) {
    const uint32_t T = (uint32_t)(frame_off[u + 1] - frame_off[u]);
    for (uint32_t t0 = 0; t0 < T; t0 += fe->span_frames) spans.push_back(make_uint2(u, t0));
  }
  if (spans.size() > 0x7FFFFFFFull) return fail(SR_ELIMIT, "%zu spans of %u frames exceed a launch's workgroups", spans.size(), fe->span_frames);
  HIP_TRY(keep->samples.upload(samples, sample_off[n_utts]));
  HIP_TRY(keep->sample_off.upload(sample_off, (size_t)n_utts + 1));
  HIP_TRY(keep->frame_off.upload(frame_off.data(), frame_off.size()));
  HIP_TRY(keep->spans.upload(spans.data(), spans.size()));
  srgpu::MfccArgs& a = keep->args;
  a.samples = keep->samples.p; a.sample_off = keep->sample_off.p; a.frame_off = keep->frame_off.p;
  a.spans = keep->spans.p; a.n_spans = (uint32_t)spans.size(); a.span_frames = fe->span_frames;
  a.window = p.window; a.shift = p.shift; a.n_fft = p.n_fft; a.n_mel = p.n_mel; a.n_cepstra = p.n_cepstra;
  a.preemphasis = p.preemphasis; a.energy_floor = p.energy_floor;
  a.win = fe->win.p; a.twiddle = fe->twiddle.p; a.mel_first = fe->mel_first.p; a.mel_count = fe->mel_count.p; a.mel_off = fe->mel_off.p;
  a.mel_w = fe->mel_w.p; a.dct = fe->dct.p;
  a.n_frames = frame_off[n_utts];
  return SR_OK;
}
// utt_warp [n_utts] (host): the utterances' warps of a warped front end; NULL: the unwarped filters
int run_mfcc(sr_frontend* fe, const int16_t* samples, const uint64_t* sample_off, uint32_t n_utts, const std::vector<uint64_t>& frame_off,
             const uint32_t* utt_warp, AudioInputs* keep, DevBuf<float>* cep) {
  const uint64_t F = frame_off[n_utts];
  HIP_TRY(cep->ensure((size_t)F * fe->mfcc.n_cepstra));
  if (F == 0) return SR_OK;
  int rc = upload_audio(fe, samples, sample_off, n_utts, frame_off, keep);
  if (rc) return rc;
  srgpu::MfccArgs a = keep->args;
  a.out = cep->p;
  if (utt_warp) {
    HIP_TRY(keep->utt_warp.upload(utt_warp, n_utts));
    a.utt_warp = keep->utt_warp.p;
    a.warp_first = fe->warp_first.p; a.warp_count = fe->warp_count.p; a.warp_off = fe->warp_off.p; a.warp_w = fe->warp_w.p;
  }
  EventPair ep{};
  if ((rc = prof_begin(fe->model, &ep))) return rc;
  HIP_TRY(srgpu::launch_mfcc(a, fe->model->s_gmm));
  return prof_end(fe->model, &ep);
}

// cepstra on the device -> a new corpus of the front end's model (the post-processing stage); waits for the stream
int corpus_of_cepstra(sr_frontend* fe, const float* d_cep, const std::vector<uint64_t>& frame_off, uint32_t n_utts, sr_corpus** out) {
  sr_model* m = fe->model;
  const sr_feature_post_params& q = fe->post;
  const uint64_t F = frame_off[n_utts];
  if ((F * m->dim + 255) / 256 > 0x7FFFFFFFull) return fail(SR_ELIMIT, "%llu frames exceed a launch's workgroups", (unsigned long long)F);
  sr_corpus* c = new sr_corpus();
  std::unique_ptr<sr_corpus, int (*)(sr_corpus*)> own(c, sr_corpus_destroy);
  c->model = m; c->n_utts = n_utts; c->n_frames = F;
  srhost::corpus_register(c);
  c->frame_off = frame_off;
  HIP_TRY(c->feats.ensure((size_t)F * m->dim + 64));
  HIP_TRY(c->d_frame_off.upload(frame_off.data(), frame_off.size()));
  srgpu::FeaturePostArgs a{};
  a.cepstra = d_cep; a.frame_off = c->d_frame_off.p; a.n_utts = n_utts; a.n_frames = F;
  a.n_static = q.n_static; a.n_first = q.n_first; a.n_second = q.n_second; a.step = q.deriv_step;
  a.mean = fe->normalise ? fe->mean.p : nullptr; a.stddev = fe->normalise ? fe->stddev.p : nullptr;
  a.energy_max_norm = q.energy_max_norm != 0;
  a.out = c->feats.p;
  EventPair ep{};
  int rc = prof_begin(m, &ep);
  if (rc) return rc;
  HIP_TRY(srgpu::launch_feature_post(a, m->s_gmm));
  if ((rc = prof_end(m, &ep))) return rc;
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  if (m->profiling) m->prof.frames += F;
  *out = own.release();
  return SR_OK;
}

// sr_frontend_create (vtln == NULL) and sr_frontend_create_warped
int create_frontend(sr_model* m, const sr_mfcc_params* mfcc, const sr_vtln_params* vtln, const sr_feature_post_params* post, sr_frontend** out) {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  if (!m) return fail(SR_EINVAL, "null model handle");
  if (!post) return fail(SR_EINVAL, "post is null");
  HIP_TRY(hipSetDevice(m->device));
  int rc;
  if (mfcc && (rc = check_mfcc(*mfcc))) return rc;
  if (post->n_static == 0) return fail(SR_EINVAL, "n_static is 0");
  if (post->n_first > post->n_static || post->n_second > post->n_first)
    return fail(SR_EINVAL, "n_first must be <= n_static and n_second <= n_first");
  if (post->deriv_step == 0) return fail(SR_EINVAL, "deriv_step is 0");
  if ((post->mean == nullptr) != (post->stddev == nullptr)) return fail(SR_EINVAL, "mean and stddev come together or not at all");
  const uint64_t nt = (uint64_t)post->n_static + post->n_first + post->n_second;
  if (nt != m->dim) return fail(SR_EINVAL, "n_static + n_first + n_second = %llu, the model has %u dimensions", (unsigned long long)nt, m->dim);
  if (mfcc && mfcc->n_cepstra != post->n_static) return fail(SR_EINVAL, "n_cepstra %u != n_static %u", mfcc->n_cepstra, post->n_static);
  if (vtln) {
    const char* what = "";
    const int bad = srplan::vtln_check(vtln->n_warps, vtln->alpha, vtln->break_frac, mfcc->n_mel, &what);
    if (bad) return fail(bad == 1 ? SR_EINVAL : SR_ELIMIT, "vtln: %s", what);
  }
  MfccTables t;
  if (mfcc && (rc = build_tables(*mfcc, vtln, &t))) return rc;
  std::unique_ptr<sr_frontend> fe(new sr_frontend());
  fe->model = m;
  fe->post = *post;
  fe->post.mean = fe->post.stddev = nullptr;
  if (post->mean) {
    fe->normalise = true;
    HIP_TRY(fe->mean.upload(post->mean, nt));
    HIP_TRY(fe->stddev.upload(post->stddev, nt));
  }
  if (mfcc) {
    fe->has_mfcc = true;
    fe->mfcc = *mfcc;
    // as many frames per workgroup as keep its samples within the LDS span (window <= n_fft <= 2048 < the span)
    const uint64_t fit = (srgpu::mfcc_span_cap() - mfcc->window) / mfcc->shift + 1;
    fe->span_frames = (uint32_t)std::min<uint64_t>(kSpanFrames, fit);
    HIP_TRY(fe->win.upload(t.win.data(), t.win.size()));
    HIP_TRY(fe->twiddle.upload(t.twiddle.data(), t.twiddle.size()));
    HIP_TRY(fe->mel_first.upload(t.mel.first.data(), t.mel.first.size()));
    HIP_TRY(fe->mel_count.upload(t.mel.count.data(), t.mel.count.size()));
    HIP_TRY(fe->mel_off.upload(t.mel.off.data(), t.mel.off.size()));
    HIP_TRY(fe->mel_w.upload(t.mel.w.data(), t.mel.w.size()));
    HIP_TRY(fe->dct.upload(t.dct.data(), t.dct.size()));
  }
  if (vtln) {
    fe->n_warps = vtln->n_warps;
    HIP_TRY(fe->warp_first.upload(t.warp.first.data(), t.warp.first.size()));
    HIP_TRY(fe->warp_count.upload(t.warp.count.data(), t.warp.count.size()));
    HIP_TRY(fe->warp_off.upload(t.warp.off.data(), t.warp.off.size()));
    HIP_TRY(fe->warp_w.upload(t.warp.w.data(), t.warp.w.size()));
  }
  *out = fe.release();
  return SR_OK;
}

// a call on a warped front end's warps: the handle, its MFCC stage, its warps
int check_warped(const sr_frontend* fe) {
  const int rc = check_frontend(fe);
  if (rc) return rc;
  if (fe->n_warps == 0) return fail(SR_EINVAL, "this front end has no warps: make it with sr_frontend_create_warped");
  return SR_OK;
}

// The warps sr_vtln_costs_corpus takes at a time on F frames in n_utts utterances (also what sr_vtln_chunks reports): as many as keep a
// chunk's cepstra, rows, replicated states and scores within the model's vtln_budget, at least one; fewer where a launch over the
// chunk's rows or its n_warps x n_utts utterances would be too large; 0: even one warp is
uint32_t vtln_chunk_warps(const sr_frontend* fe, uint64_t F, uint32_t n_utts) {
  const sr_model* m = fe->model;
  const uint32_t W = fe->n_warps;
  const uint64_t per_warp = F * (sizeof(float) * ((uint64_t)fe->mfcc.n_cepstra + m->dim) + sizeof(uint16_t) + sizeof(double));
  uint32_t Wc = (uint32_t)std::min<uint64_t>(W, std::max<uint64_t>(1, per_warp ? m->vtln_budget / per_warp : W));
  auto fits = [&](uint64_t w) { return (w * F * m->dim + 255) / 256 <= 0x7FFFFFFFull && w * n_utts <= 0xFFFFFFFEull; };
  while (Wc > 1 && !fits(Wc)) Wc--;
  return fits(Wc) ? Wc : 0;
}

}  // namespace

extern "C" {

int sr_vtln_chunks(const sr_frontend* fe, uint64_t n_frames, uint32_t n_utts, uint32_t* out_chunks) {
  return guarded(__func__, [&]() -> int {
  if (!fe || !fe->model) return fail(SR_EINVAL, "null front end handle");
  if (fe->n_warps == 0) return fail(SR_EINVAL, "this front end has no warps: make it with sr_frontend_create_warped");
  if (!out_chunks) return fail(SR_EINVAL, "out_chunks is null");
  const uint32_t Wc = vtln_chunk_warps(fe, n_frames, n_utts);
  if (Wc == 0) return fail(SR_ELIMIT, "%llu frames in %u utterances exceed a launch's workgroups", (unsigned long long)n_frames, n_utts);
  *out_chunks = (fe->n_warps + Wc - 1) / Wc;
  return SR_OK;
  });
}

int sr_frontend_create(sr_model* m, const sr_mfcc_params* mfcc, const sr_feature_post_params* post, sr_frontend** out) {
  return guarded(__func__, [&]() -> int { return create_frontend(m, mfcc, nullptr, post, out); });
}

int sr_frontend_create_warped(sr_model* m, const sr_mfcc_params* mfcc, const sr_vtln_params* vtln, const sr_feature_post_params* post,
                              sr_frontend** out) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  if (!mfcc) return fail(SR_EINVAL, "mfcc is null: a warped front end has an MFCC stage");
  if (!vtln) return fail(SR_EINVAL, "vtln is null");
  return create_frontend(m, mfcc, vtln, post, out);
  });
}

int sr_frontend_warps(const sr_frontend* fe, uint32_t* n_warps) {
  return guarded(__func__, [&]() -> int {
  if (!fe) return fail(SR_EINVAL, "null front end handle");
  if (!n_warps) return fail(SR_EINVAL, "n_warps is null");
  *n_warps = fe->n_warps;
  return SR_OK;
  });
}

int sr_frontend_destroy(sr_frontend* fe) {
  return guarded(__func__, [&]() -> int {
  if (!fe) return SR_OK;
  if (fe->model) { (void)hipSetDevice(fe->model->device); (void)hipDeviceSynchronize(); }
  delete fe;  // (the tables go with it)
  return SR_OK;
  });
}

int sr_frontend_frames(const sr_frontend* fe, uint64_t n_samples, uint64_t* frames) {
  return guarded(__func__, [&]() -> int {
  if (!fe) return fail(SR_EINVAL, "null front end handle");
  if (!frames) return fail(SR_EINVAL, "frames is null");
  if (!fe->has_mfcc) return fail(SR_EINVAL, "this front end was made without an MFCC stage");
  *frames = frames_of(fe->mfcc, n_samples);
  return SR_OK;
  });
}

int sr_corpus_from_audio(sr_frontend* fe, const int16_t* samples, const uint64_t* sample_off, uint32_t n_utts, sr_corpus** out,
                         uint64_t* out_frame_off) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  int rc = check_frontend(fe);
  if (rc) return rc;
  if (!out_frame_off) return fail(SR_EINVAL, "out_frame_off is null");
  std::vector<uint64_t> frame_off;
  if ((rc = check_audio(fe, samples, sample_off, n_utts, &frame_off))) return rc;
  AudioInputs keep;
  DevBuf<float> cep;
  if ((rc = run_mfcc(fe, samples, sample_off, n_utts, frame_off, nullptr, &keep, &cep))) return rc;
  if ((rc = corpus_of_cepstra(fe, cep.p, frame_off, n_utts, out))) return rc;
  std::memcpy(out_frame_off, frame_off.data(), sizeof(uint64_t) * frame_off.size());
  return SR_OK;
  });
}

int sr_corpus_from_audio_warped(sr_frontend* fe, const int16_t* samples, const uint64_t* sample_off, uint32_t n_utts, const uint32_t* utt_warp,
                                sr_corpus** out, uint64_t* out_frame_off) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  int rc = check_warped(fe);
  if (rc) return rc;
  if (!out_frame_off) return fail(SR_EINVAL, "out_frame_off is null");
  std::vector<uint64_t> frame_off;
  if ((rc = check_audio(fe, samples, sample_off, n_utts, &frame_off))) return rc;
  if (n_utts > 0 && !utt_warp) return fail(SR_EINVAL, "utt_warp is null");
  for (uint32_t u = 0; u < n_utts; u++)
    if (utt_warp[u] >= fe->n_warps) return fail(SR_EINVAL, "utterance %u: warp %u >= n_warps %u", u, utt_warp[u], fe->n_warps);
  AudioInputs keep;
  DevBuf<float> cep;
  if ((rc = run_mfcc(fe, samples, sample_off, n_utts, frame_off, n_utts ? utt_warp : nullptr, &keep, &cep))) return rc;
  if ((rc = corpus_of_cepstra(fe, cep.p, frame_off, n_utts, out))) return rc;
  std::memcpy(out_frame_off, frame_off.data(), sizeof(uint64_t) * frame_off.size());
  return SR_OK;
  });
}

int sr_vtln_costs_corpus(sr_frontend* fe, const int16_t* samples, const uint64_t* sample_off, uint32_t n_utts, const uint16_t* states,
                         const uint32_t* utt_speaker, uint32_t n_speakers, double* out_cost, uint64_t* out_frames) {
  return guarded(__func__, [&]() -> int {
  int rc = check_warped(fe);
  if (rc) return rc;
  sr_model* m = fe->model;
  const sr_mfcc_params& p = fe->mfcc;
  const uint32_t W = fe->n_warps, S = n_speakers;
  if (S > 0 && (!out_cost || !out_frames)) return fail(SR_EINVAL, "out_cost or out_frames is null");
  std::vector<uint64_t> frame_off;
  if ((rc = check_audio(fe, samples, sample_off, n_utts, &frame_off))) return rc;
  const uint64_t F = frame_off[n_utts];
  if (F > 0 && !states) return fail(SR_EINVAL, "states is null");
  if (n_utts > 0 && !utt_speaker) return fail(SR_EINVAL, "utt_speaker is null");
  for (uint64_t f = 0; f < F; f++)
    if (states[f] >= m->n_states) return fail(SR_EINVAL, "frame %llu: state %u >= n_states", (unsigned long long)f, states[f]);
  // a speaker's utterances in ascending order, and its frames
  std::vector<uint64_t> spk_off((size_t)S + 1, 0), frames(S, 0);
  for (uint32_t u = 0; u < n_utts; u++) {
    if (utt_speaker[u] >= S) return fail(SR_EINVAL, "utterance %u: speaker %u >= n_speakers %u", u, utt_speaker[u], S);
    spk_off[utt_speaker[u] + 1]++;
    frames[utt_speaker[u]] += frame_off[u + 1] - frame_off[u];
  }
  for (uint32_t s = 0; s < S; s++) spk_off[s + 1] += spk_off[s];
  std::vector<uint32_t> spk_utt(n_utts);
  {
    std::vector<uint64_t> next(spk_off.begin(), spk_off.end() - 1);
    for (uint32_t u = 0; u < n_utts; u++) spk_utt[next[utt_speaker[u]]++] = u;
  }
  const uint32_t Wc = vtln_chunk_warps(fe, F, n_utts);
  if (Wc == 0) return fail(SR_ELIMIT, "%llu frames in %u utterances exceed a launch's workgroups", (unsigned long long)F, n_utts);
  if (S == 0) return SR_OK;
  std::vector<double> cost((size_t)S * W, 0.0);
  if (F > 0) {
    AudioInputs keep;
    if ((rc = upload_audio(fe, samples, sample_off, n_utts, frame_off, &keep))) return rc;
    // the chunk as a corpus of Wc x n_utts utterances: its frame offsets, and the alignment once per warp
    std::vector<uint64_t> rep_off((size_t)Wc * n_utts + 1);
    std::vector<uint16_t> rep_states((size_t)Wc * F);
    for (uint32_t w = 0; w < Wc; w++) {
      for (uint32_t u = 0; u < n_utts; u++) rep_off[(size_t)w * n_utts + u] = w * F + frame_off[u];
      std::memcpy(rep_states.data() + (size_t)w * F, states, sizeof(uint16_t) * F);
    }
    rep_off[(size_t)Wc * n_utts] = Wc * F;
    DevBuf<uint64_t> d_rep_off, d_spk_off;
    DevBuf<uint16_t> d_states;
    DevBuf<uint32_t> d_spk_utt;
    DevBuf<float> cep, rows;
    DevBuf<double> scores, utt_cost, d_cost;
    HIP_TRY(d_rep_off.upload(rep_off.data(), rep_off.size()));
    HIP_TRY(d_states.upload(rep_states.data(), rep_states.size()));
    HIP_TRY(d_spk_off.upload(spk_off.data(), spk_off.size()));
    HIP_TRY(d_spk_utt.upload(spk_utt.data(), spk_utt.size()));
    HIP_TRY(cep.ensure((size_t)Wc * F * p.n_cepstra));
    HIP_TRY(rows.ensure((size_t)Wc * F * m->dim + 64));
    HIP_TRY(scores.ensure((size_t)Wc * F));
    HIP_TRY(utt_cost.ensure((size_t)W * n_utts));
    HIP_TRY(d_cost.ensure((size_t)S * W));
    // SRGPU_VTLN_TIMING (include/srgpu.h; read when the model was made): the chunk count and the stages' HIP-event times to stderr
    const bool timing = m->vtln_timing;
    struct Marks {
      std::vector<hipEvent_t> e;
      ~Marks() { for (hipEvent_t x : e) (void)hipEventDestroy(x); }  // on every way out
    } marks_owner;
    std::vector<hipEvent_t>& marks = marks_owner.e;
    auto mark = [&]() -> hipError_t {
      if (!timing) return hipSuccess;
      hipEvent_t e;
      hipError_t err = hipEventCreate(&e);
      if (err != hipSuccess) return err;
      marks.push_back(e);
      return hipEventRecord(e, m->s_gmm);
    };
    EventPair ep{};
    if ((rc = prof_begin(m, &ep))) return rc;
    for (uint32_t a0 = 0; a0 < W; a0 += Wc) {
      const uint32_t nw = std::min(Wc, W - a0);
      HIP_TRY(mark());
      srgpu::MfccArgs a = keep.args;
      a.out = cep.p; a.n_warps = nw;
      a.warp_first = fe->warp_first.p + (size_t)a0 * p.n_mel; a.warp_count = fe->warp_count.p + (size_t)a0 * p.n_mel;
      a.warp_off = fe->warp_off.p + (size_t)a0 * p.n_mel; a.warp_w = fe->warp_w.p;
      HIP_TRY(srgpu::launch_mfcc_warps(a, m->s_gmm));
      HIP_TRY(mark());
      const sr_feature_post_params& q = fe->post;
      srgpu::FeaturePostArgs fp{};
      fp.cepstra = cep.p; fp.frame_off = d_rep_off.p; fp.n_utts = nw * n_utts; fp.n_frames = nw * F;
      fp.n_static = q.n_static; fp.n_first = q.n_first; fp.n_second = q.n_second; fp.step = q.deriv_step;
      fp.mean = fe->normalise ? fe->mean.p : nullptr; fp.stddev = fe->normalise ? fe->stddev.p : nullptr;
      fp.energy_max_norm = q.energy_max_norm != 0;
      fp.out = rows.p;
      HIP_TRY(srgpu::launch_feature_post(fp, m->s_gmm));
      HIP_TRY(mark());
      srgpu::EmArgs e{};
      e.feats = rows.p; e.n_frames = nw * F; e.dim = m->dim; e.states = d_states.p;
      e.dens_off = m->dens_off.p; e.means = m->means.p; e.inv_vars = m->inv_vars.p; e.norm = m->norm.p; e.logw = m->logw.p;
      e.max_approx = m->max_approx;
      HIP_TRY(srgpu::launch_path_scores_direct(e, scores.p, m->s_gmm));
      HIP_TRY(mark());
      srgpu::VtlnReduceArgs r{};
      r.src = scores.p; r.src_stride = F; r.off = keep.frame_off.p; r.items = nullptr; r.n_rows = n_utts; r.n_warps = nw;
      r.out = utt_cost.p + (size_t)a0 * n_utts; r.out_row = 1; r.out_warp = n_utts;
      HIP_TRY(srgpu::launch_vtln_reduce(r, m->s_gmm));
      HIP_TRY(mark());
    }
    srgpu::VtlnReduceArgs r{};
    r.src = utt_cost.p; r.src_stride = n_utts; r.off = d_spk_off.p; r.items = d_spk_utt.p; r.n_rows = S; r.n_warps = W;
    r.out = d_cost.p; r.out_row = W; r.out_warp = 1;
    HIP_TRY(srgpu::launch_vtln_reduce(r, m->s_gmm));
    HIP_TRY(mark());
    if ((rc = prof_end(m, &ep))) return rc;
    HIP_TRY(hipStreamSynchronize(m->s_gmm));
    HIP_TRY(hipMemcpy(cost.data(), d_cost.p, sizeof(double) * cost.size(), hipMemcpyDeviceToHost));
    if (timing) {  // marks: five per chunk -- before the MFCC stage, after it, after the post-processing, scoring, reduction -- and the end
      float t[4] = {0, 0, 0, 0}, ms = 0.0f;
      for (size_t i = 0; i + 1 < marks.size(); i++) {
        HIP_TRY(hipEventElapsedTime(&ms, marks[i], marks[i + 1]));
        if (i % 5 < 4) t[i % 5] += ms; else t[3] += ms;
      }
      fprintf(stderr, "vtln_timing chunks %u mfcc_warps_ms %.4f post_ms %.4f score_ms %.4f reduce_ms %.4f\n", (W + Wc - 1) / Wc, t[0], t[1], t[2], t[3]);
    }
    if (m->profiling) m->prof.frames += F;
  }
  std::memcpy(out_cost, cost.data(), sizeof(double) * cost.size());
  std::memcpy(out_frames, frames.data(), sizeof(uint64_t) * S);
  return SR_OK;
  });
}

int sr_corpus_from_cepstra(sr_frontend* fe, const float* cepstra, const uint64_t* frame_off, uint32_t n_utts, sr_corpus** out) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  int rc = check_frontend(fe);
  if (rc) return rc;
  if ((rc = check_offsets(frame_off, n_utts, "frame_off")) || (rc = check_frame_counts(frame_off, n_utts))) return rc;
  const uint64_t F = frame_off[n_utts];
  if (F > 0 && !cepstra) return fail(SR_EINVAL, "cepstra is null");
  DevBuf<float> cep;
  HIP_TRY(cep.upload(cepstra, (size_t)F * fe->post.n_static));
  return corpus_of_cepstra(fe, cep.p, std::vector<uint64_t>(frame_off, frame_off + n_utts + 1), n_utts, out);
  });
}

int sr_mfcc_corpus(sr_frontend* fe, const int16_t* samples, const uint64_t* sample_off, uint32_t n_utts, float* out_cepstra,
                   uint64_t* out_frame_off) {
  return guarded(__func__, [&]() -> int {
  int rc = check_frontend(fe);
  if (rc) return rc;
  if (!out_frame_off) return fail(SR_EINVAL, "out_frame_off is null");
  std::vector<uint64_t> frame_off;
  if ((rc = check_audio(fe, samples, sample_off, n_utts, &frame_off))) return rc;
  const uint64_t F = frame_off[n_utts];
  if (F > 0 && !out_cepstra) return fail(SR_EINVAL, "out_cepstra is null");
  AudioInputs keep;
  DevBuf<float> cep;
  if ((rc = run_mfcc(fe, samples, sample_off, n_utts, frame_off, nullptr, &keep, &cep))) return rc;
  HIP_TRY(hipStreamSynchronize(fe->model->s_gmm));
  if (F > 0) HIP_TRY(hipMemcpy(out_cepstra, cep.p, sizeof(float) * (size_t)F * fe->mfcc.n_cepstra, hipMemcpyDeviceToHost));
  std::memcpy(out_frame_off, frame_off.data(), sizeof(uint64_t) * frame_off.size());
  return SR_OK;
  });
}

int sr_corpus_download(sr_corpus* c, float* out) {
  return guarded(__func__, [&]() -> int {
  if (!c || !c->model) return fail(SR_EINVAL, "null corpus handle");
  if (c->n_frames > 0 && !out) return fail(SR_EINVAL, "out is null");
  HIP_TRY(hipSetDevice(c->model->device));
  const int rc = sr_corpus_wait(c);  // an asynchronous upload: all of it
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (c->n_frames > 0)
    HIP_TRY(hipMemcpy(out, c->feats.p, sizeof(float) * (size_t)c->n_frames * c->model->dim, hipMemcpyDeviceToHost));
  return SR_OK;
  });
}

}  // extern "C"
