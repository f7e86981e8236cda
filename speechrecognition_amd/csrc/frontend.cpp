// frontend.cpp -- the host side of the audio front end (include/srgpu.h: sr_frontend_*, sr_corpus_from_audio, sr_corpus_from_cepstra,
// sr_mfcc_corpus, sr_corpus_download): the argument checks, the MFCC stage's tables -- computed in double, stored as float -- and the
// entry points.  The kernels are frontend.hip.
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "handles.h"

using srhost::fail;
using srhost::guarded;

namespace {

constexpr uint32_t kSpanFrames = 16;  // most frames a workgroup of mfcc_kernel covers

double mel(double f) { return 2595.0 * std::log10(1.0 + f / 700.0); }
double mel_inv(double m) { return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0); }

struct MfccTables {
  std::vector<float> win, mel_w, dct;
  std::vector<float2> twiddle;
  std::vector<uint32_t> mel_first, mel_count, mel_off;
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

// the tables of include/srgpu.h's definition; SR_EINVAL for a filter without a bin of positive weight
int build_tables(const sr_mfcc_params& p, MfccTables* t) {
  const double pi = 3.14159265358979323846;
  const uint32_t N = p.n_fft, bins = N / 2 + 1;
  t->win.resize(p.window);
  for (uint32_t i = 0; i < p.window; i++) t->win[i] = (float)(0.54 - 0.46 * std::cos(2.0 * pi * i / (p.window - 1)));
  t->twiddle.resize(N);
  for (uint32_t n = 0; n < N; n++) {
    const double ang = 2.0 * pi * n / N;
    t->twiddle[n] = make_float2((float)std::cos(ang), (float)-std::sin(ang));
  }
  const double lo = mel(p.f_low), hi = mel(p.f_high), step = (hi - lo) / (p.n_mel + 1);
  std::vector<double> edge(p.n_mel + 2);
  for (uint32_t j = 0; j < p.n_mel + 2; j++) edge[j] = mel_inv(lo + j * step);
  t->mel_first.assign(p.n_mel, 0);
  t->mel_count.assign(p.n_mel, 0);
  t->mel_off.assign(p.n_mel, 0);
  t->mel_w.clear();
  for (uint32_t m = 0; m < p.n_mel; m++) {
    const double l = edge[m], c = edge[m + 1], r = edge[m + 2];
    uint32_t first = bins, last = 0;  // the bins of positive weight: first .. last
    std::vector<float> w(bins, 0.0f);
    for (uint32_t k = 0; k < bins; k++) {
      const double fk = k * (p.sample_rate / N);
      const double v = std::max(0.0, std::min((fk - l) / (c - l), (r - fk) / (r - c)));
      w[k] = (float)v;
      if (w[k] > 0.0f) { first = std::min(first, k); last = k; }
    }
    if (first == bins) return fail(SR_EINVAL, "mfcc: filter %u (%.1f .. %.1f Hz) has no bin of positive weight", m, l, r);
    t->mel_first[m] = first;
    t->mel_count[m] = last - first + 1;
    t->mel_off[m] = (uint32_t)t->mel_w.size();
    t->mel_w.insert(t->mel_w.end(), w.begin() + first, w.begin() + last + 1);
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

// samples -> static cepstra on the device, cep [frames x n_cepstra]; queued on the model's scoring stream, not waited for.  `keep`
// holds the launch's inputs until the caller has synchronised
struct AudioInputs {
  DevBuf<int16_t> samples;
  DevBuf<uint64_t> sample_off, frame_off;
  DevBuf<uint2> spans;
};
int run_mfcc(sr_frontend* fe, const int16_t* samples, const uint64_t* sample_off, uint32_t n_utts, const std::vector<uint64_t>& frame_off,
             AudioInputs* keep, DevBuf<float>* cep) {
  const sr_mfcc_params& p = fe->mfcc;
  const uint64_t F = frame_off[n_utts];
  HIP_TRY(cep->ensure((size_t)F * p.n_cepstra));
  if (F == 0) return SR_OK;
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
  srgpu::MfccArgs a{};
  a.samples = keep->samples.p; a.sample_off = keep->sample_off.p; a.frame_off = keep->frame_off.p;
  a.spans = keep->spans.p; a.n_spans = (uint32_t)spans.size(); a.span_frames = fe->span_frames;
  a.window = p.window; a.shift = p.shift; a.n_fft = p.n_fft; a.n_mel = p.n_mel; a.n_cepstra = p.n_cepstra;
  a.preemphasis = p.preemphasis; a.energy_floor = p.energy_floor;
  a.win = fe->win.p; a.twiddle = fe->twiddle.p; a.mel_first = fe->mel_first.p; a.mel_count = fe->mel_count.p; a.mel_off = fe->mel_off.p;
  a.mel_w = fe->mel_w.p; a.dct = fe->dct.p; a.out = cep->p;
  EventPair ep{};
  int rc = prof_begin(fe->model, &ep);
  if (rc) return rc;
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

}  // namespace

extern "C" {

int sr_frontend_create(sr_model* m, const sr_mfcc_params* mfcc, const sr_feature_post_params* post, sr_frontend** out) {
  return guarded(__func__, [&]() -> int {
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
  MfccTables t;
  if (mfcc && (rc = build_tables(*mfcc, &t))) return rc;
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
    HIP_TRY(fe->mel_first.upload(t.mel_first.data(), t.mel_first.size()));
    HIP_TRY(fe->mel_count.upload(t.mel_count.data(), t.mel_count.size()));
    HIP_TRY(fe->mel_off.upload(t.mel_off.data(), t.mel_off.size()));
    HIP_TRY(fe->mel_w.upload(t.mel_w.data(), t.mel_w.size()));
    HIP_TRY(fe->dct.upload(t.dct.data(), t.dct.size()));
  }
  *out = fe.release();
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
  if ((rc = run_mfcc(fe, samples, sample_off, n_utts, frame_off, &keep, &cep))) return rc;
  if ((rc = corpus_of_cepstra(fe, cep.p, frame_off, n_utts, out))) return rc;
  std::memcpy(out_frame_off, frame_off.data(), sizeof(uint64_t) * frame_off.size());
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
  if ((rc = run_mfcc(fe, samples, sample_off, n_utts, frame_off, &keep, &cep))) return rc;
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
