// Host runtime of the MI355X tracking engine: HBM layout of the activations, frame staging, the launch of a frame
// (optionally one hipGraph per batch shape), tracker state and the engine's C ABI of mmtrack.h.
// (weights: engine_weights.cpp; the launch sequence: engine_forward.cpp; the operator entry points: ops_api.cpp)
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "engine.h"

using namespace mmt;

namespace {

int alloc_acts(mmt_engine* e) {
  const int B = e->cfg.max_batch;
  struct Req { void** p; size_t bytes; };
  std::vector<Req> reqs;
  const bool exists[4] = {true, e->ce_mask, e->split, e->cfg.debug_outputs != 0};   // by ActWhen
  auto add = [&](ActWhen group) {
    for_each_act(e->acts, e, [&](auto*& p, size_t per, ActIndex, ActWhen when, int planes) {
      if (when == group && exists[when]) reqs.push_back({(void**)&p, (size_t)planes * B * per * sizeof(*p)});
    });
  };
  // the carving order is part of the layout: the one-off buffers sit between the groups of the table
  add(ALWAYS);
  reqs.push_back({(void**)&e->zero, 256});
  add(IF_CE_MASK);
  reqs.push_back({(void**)&e->hring.ctr, 256});   // ctr, cur
  reqs.push_back({(void**)&e->splitk_ws, (size_t)mmt_engine::kMaxParts * kSplitKWsElems * 4});
  add(IF_SPLIT);
  add(IF_DEBUG);
  e->acts.half8 = (size_t)B * e->L * 8;
  size_t total = 0;
  for (auto& r : reqs) total += (r.bytes + 255) & ~size_t(255);
  HIPCHECK(e, hipMalloc(&e->aarena, total));
  HIPCHECK(e, hipMemset(e->aarena, 0, total));
  size_t off = 0;
  for (auto& r : reqs) {
    *r.p = static_cast<char*>(e->aarena) + off;
    off += (r.bytes + 255) & ~size_t(255);
  }
  if (e->ce_mask) {   // ALL: every template token of every slot
    std::vector<int> rows((size_t)B * e->Lz), nrows(B, e->Lz);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = (int)(i % e->Lz);
    HIPCHECK(e, hipMemcpy(e->acts.ce_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
    HIPCHECK(e, hipMemcpy(e->acts.ce_nrows, nrows.data(), nrows.size() * 4, hipMemcpyHostToDevice));
  }
  // the ring is read / written by kernels in place: fine-grained coherent pinned memory, so no GPU cache
  // holds a stale copy of an entry between the launches that reuse it (frame pointer / size may change)
  constexpr unsigned kRingFlags = hipHostMallocMapped | hipHostMallocCoherent;
  HIPCHECK(e, hipHostMalloc((void**)&e->params_host, (size_t)kRing * B * sizeof(CropParam), kRingFlags));
  HIPCHECK(e, hipHostMalloc((void**)&e->outs_host, (size_t)kRing * B * sizeof(TrackOut), kRingFlags));
  e->hring.cur = e->hring.ctr + 1;
  e->hring.kring = kRing;
  e->hring.pitch = B;
  e->ring_handoff = getenv("MMT_RING_COPY") == nullptr;   // tuning / A-B: copy launches instead
  HIPCHECK(e, hipHostGetDevicePointer((void**)&e->hring.params, e->params_host, 0));
  HIPCHECK(e, hipHostGetDevicePointer((void**)&e->hring.outs, e->outs_host, 0));
  for (auto& t : e->ring) HIPCHECK(e, hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
  return MMT_OK;
}

// crop geometry of processing_utils.py:32-41 in doubles with Python rounding (round half to even)
int geometry(mmt_engine* e, const double box[4], double factor, int out_sz, int* x1, int* y1, int* crop_sz,
             double* rf) {
  const int rc = mmt_crop_geometry_host(box, factor, out_sz, x1, y1, crop_sz, rf);   // the host's one copy
  if (rc == MMT_E_BOX) return e->fail(MMT_E_BOX, "Too small bounding box.");
  if (rc) return e->fail(MMT_E_ARG, "crop size out of range");
  return MMT_OK;
}

int stage_frame(mmt_engine* e, int slot, int ring, const uint8_t* frame, int Hh, int Ww, int Cc, int64_t stride,
                int is_device, const uint8_t** dev, hipStream_t cs) {
  if (!frame || Hh < 2 || Ww < 2 || Cc != e->cfg.in_chans || stride < (int64_t)Ww * Cc)
    return e->fail(MMT_E_ARG, "bad frame (expect H x W x in_chans uint8, H,W >= 2)");
  if (is_device) {
    *dev = frame;
    return MMT_OK;
  }
  const size_t bytes = (size_t)stride * Hh;
  const size_t k = (size_t)slot * kRing + ring;
  if (e->frame_cap[k] < bytes) {
    if (e->frame_dev[k]) {
      HIPCHECK(e, hipStreamSynchronize(e->stream));
      HIPCHECK(e, hipStreamSynchronize(cs));
      hipFree(e->frame_dev[k]);
    }
    e->frame_dev[k] = nullptr;
    HIPCHECK(e, hipMalloc(&e->frame_dev[k], bytes));
    e->frame_cap[k] = bytes;
  }
  HIPCHECK(e, hipMemcpyAsync(e->frame_dev[k], frame, bytes, hipMemcpyHostToDevice, cs));
  *dev = e->frame_dev[k];
  return MMT_OK;
}

int launch(mmt_engine* e, int b0, int n, const GraphEntry** replayed) {
  *replayed = nullptr;
  // HIP does not time event-record nodes captured into a graph, so the kernel timing probe runs the
  // identical launch sequence eagerly, bracketing the probed kernel class with stream events
  if (!e->cfg.use_graphs || e->probe) {
    if (!enqueue_split(e, b0, n)) return MMT_E_ARG;
    ++e->launches;
    HIPCHECK(e, hipGetLastError());
    return MMT_OK;
  }
  const std::string pc = e->probe ? e->probe->cls : std::string();
  auto key = std::make_tuple(b0, n, pc);
  auto it = e->graphs.find(key);
  if (it == e->graphs.end()) {
    // first use of this batch shape: run eagerly (validates every launch, yields this frame's
    // result), then capture the identical launch sequence for replay
    TimingProbe* p = e->probe.get();
    if (p) {
      p->used = 0;
      p->pending_work.clear();
    }
    if (!enqueue_split(e, b0, n)) return MMT_E_ARG;
    ++e->launches;
    HIPCHECK(e, hipGetLastError());
    GraphEntry entry;
    if (p) p->capture = &entry;
    hipGraph_t g;
    hipError_t st = hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal);
    if (st == hipSuccess) {
      enqueue_split(e, b0, n);   // the same GEMMs as the eager pass above: it cannot fail here
      st = hipStreamEndCapture(e->stream, &g);
    }
    if (p) p->capture = nullptr;
    if (st != hipSuccess) return e->fail(MMT_E_HIP, std::string("graph capture: ") + hipGetErrorString(st));
    HIPCHECK(e, hipGraphInstantiate(&entry.exec, g, nullptr, nullptr, 0));
    hipGraphDestroy(g);
    e->graphs.emplace(key, std::move(entry));
    return MMT_OK;
  }
  HIPCHECK(e, hipGraphLaunch(it->second.exec, e->stream));
  ++e->launches;
  *replayed = &it->second;
  return MMT_OK;
}

// every captured graph and its probe events (the weights, or a kernel argument the graphs carry, changed)
void drop_graphs(mmt_engine* e) {
  for (auto& kv : e->graphs) {
    hipGraphExecDestroy(kv.second.exec);
    for (auto& pr : kv.second.ev) {
      hipEventDestroy(pr.first);
      hipEventDestroy(pr.second);
    }
  }
  e->graphs.clear();
}

// the host copy of slot's state -> its device-resident copy (stream-ordered, synchronous)
int write_state(mmt_engine* e, int slot) {
  SeqState st{};
  for (int k = 0; k < 4; ++k) st.box[k] = e->state[slot][k];
  st.rf = 1.0;
  HIPCHECK(e, hipMemcpyAsync(e->acts.state_dev + slot, &st, sizeof(SeqState), hipMemcpyHostToDevice, e->stream));
  HIPCHECK(e, hipStreamSynchronize(e->stream));
  return MMT_OK;
}

int check_engine(mmt_engine* e) {
  if (!e) return MMT_E_ARG;
  if (!e->finalized) return e->fail(MMT_E_STATE, "engine not finalized (load every state_dict key first)");
  HIPCHECK(e, hipSetDevice(e->device));
  return MMT_OK;
}

}  // namespace

// =================================================================== C ABI
extern "C" {

const char* mmt_version(void) { return "mmtrack-mi355x 0.1 (gfx950)"; }
int mmt_abi_version(void) { return MMT_ABI_VERSION; }
void* mmt_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (!bytes || hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return nullptr;
  return p;
}
void mmt_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int mmt_create(const mmt_config* cfg, int device, mmt_engine** out) {
  if (!cfg || !out) return MMT_E_ARG;
  *out = nullptr;
  auto e = std::make_unique<mmt_engine>();
  e->cfg = *cfg;
  e->device = device;
  const auto& c = e->cfg;
  if (c.template_size % 16 || c.search_size % 16 || c.template_size <= 0 || c.search_size <= 0 ||
      c.max_batch <= 0 || c.n_ce < 0 || c.n_ce > 12 || c.head_channels != 256 ||
      (c.model == MMT_MODEL_VIPT && (c.in_chans != 6 || c.prompt_type == MMT_PROMPT_NONE)) ||
      (c.model == MMT_MODEL_OSTRACK && c.in_chans != 3)) {
    *out = nullptr;
    return MMT_E_ARG;
  }
  e->Lz = (c.template_size / 16) * (c.template_size / 16);
  e->Lx = (c.search_size / 16) * (c.search_size / 16);
  e->L = e->Lz + e->Lx;
  e->fs = c.search_size / 16;
  e->tfs = c.template_size / 16;
  e->ce_mask = c.ce_template_index == MMT_CE_TEMPLATE_MASK;
  if (e->L > 1024 || (c.n_ce > 0 && !e->ce_mask && (c.ce_template_index < 0 || c.ce_template_index >= e->Lz)))
    return MMT_E_ARG;
  if (c.precision < 0 || c.precision > 1) return MMT_E_ARG;
  e->split = c.precision == 1;
  e->nprompt = c.model == MMT_MODEL_VIPT ? (c.prompt_type == MMT_PROMPT_DEEP ? DEPTH : (c.prompt_type ? 1 : 0)) : 0;
  int Ls = e->Lx;
  for (int i = 0; i < DEPTH; ++i) {
    e->ls_before.push_back(Ls);
    for (int k = 0; k < c.n_ce; ++k)
      if (c.ce_loc[k] == i) {
        const int keep = (int)std::ceil(c.ce_keep_ratio[k] * Ls);  // attn_blocks.py:40
        if (keep < Ls && keep > 0) Ls = keep;
      }
    e->keep_at.push_back(Ls);
  }
  if (hipSetDevice(device) != hipSuccess) return MMT_E_HIP;
  if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) return MMT_E_HIP;
  for (auto& xs : e->xstream)
    if (hipStreamCreateWithFlags(&xs, hipStreamNonBlocking) != hipSuccess) return MMT_E_HIP;
  if (hipStreamCreateWithFlags(&e->cstream, hipStreamNonBlocking) != hipSuccess) return MMT_E_HIP;
  for (auto& ev : e->copy_ev)
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return MMT_E_HIP;
  if (hipEventCreateWithFlags(&e->frame_ev, hipEventDisableTiming) != hipSuccess) return MMT_E_HIP;
  for (auto& je : e->join_ev)
    if (hipEventCreateWithFlags(&je, hipEventDisableTiming) != hipSuccess) return MMT_E_HIP;
  if (hipEventCreateWithFlags(&e->fork_ev, hipEventDisableTiming) != hipSuccess)
    return MMT_E_HIP;
  // f16x3 GEMMs are 3x longer, so halves of 16 sequences still fill the chip and the two streams fill each
  // other's tile-quantisation tails (+8 % at 32 sequences; plain bf16 lost 4 % there)
  if (e->split) e->overlap_min = 32;
  if (const char* ov = std::getenv("MMT_OVERLAP_MIN")) e->overlap_min = std::atoi(ov);
  if (const char* np = std::getenv("MMT_NPARTS")) e->nparts = std::min(std::max(std::atoi(np), 2), mmt_engine::kMaxParts);
  build_expected(e.get());
  e->frame_dev.assign((size_t)c.max_batch * kRing, nullptr);
  e->frame_cap.assign((size_t)c.max_batch * kRing, 0);
  e->state.assign(c.max_batch, {0, 0, 0, 0});
  e->active.assign(c.max_batch, 0);
  if (alloc_acts(e.get()) != MMT_OK) return MMT_E_HIP;
  *out = e.release();
  return MMT_OK;
}

void mmt_destroy(mmt_engine* e) {
  if (!e) return;
  hipSetDevice(e->device);
  hipStreamSynchronize(e->stream);
  drop_graphs(e);
  if (e->probe)
    for (auto& p : e->probe->ev) {
      hipEventDestroy(p.first);
      hipEventDestroy(p.second);
    }
  for (auto* p : e->frame_dev)
    if (p) hipFree(p);
  if (e->warena) hipFree(e->warena);
  if (e->aarena) hipFree(e->aarena);
  if (e->params_host) hipHostFree(e->params_host);
  if (e->outs_host) hipHostFree(e->outs_host);
  for (auto& t : e->ring)
    if (t.done) hipEventDestroy(t.done);
  if (e->stream) hipStreamDestroy(e->stream);
  for (auto& xs : e->xstream)
    if (xs) hipStreamDestroy(xs);
  if (e->cstream) {
    hipStreamSynchronize(e->cstream);
    hipStreamDestroy(e->cstream);
  }
  for (auto& ev : e->copy_ev)
    if (ev) hipEventDestroy(ev);
  if (e->frame_ev) hipEventDestroy(e->frame_ev);
  if (e->fork_ev) hipEventDestroy(e->fork_ev);
  for (auto& je : e->join_ev)
    if (je) hipEventDestroy(je);
  delete e;
}

const char* mmt_last_error(const mmt_engine* e) { return e ? e->err.c_str() : "null engine"; }

int mmt_num_expected_keys(const mmt_engine* e) { return e ? (int)e->expected_order.size() : 0; }
const char* mmt_expected_key(const mmt_engine* e, int i) {
  return (e && i >= 0 && i < (int)e->expected_order.size()) ? e->expected_order[i].c_str() : nullptr;
}

int mmt_set_tensor(mmt_engine* e, const char* key, const float* data, const int64_t* shape, int ndim) {
  if (!e || !key || (!data && ndim > 0)) return MMT_E_ARG;
  auto it = e->expected.find(key);
  if (it == e->expected.end()) return e->fail(MMT_E_WEIGHTS, std::string("Unexpected key(s) in state_dict: ") + key);
  std::vector<int64_t> shp(shape, shape + ndim);
  if (shp != it->second) return e->fail(MMT_E_WEIGHTS, std::string("size mismatch for ") + key);
  int64_t n = 1;
  for (auto d : shp) n *= d;
  HostTensor t;
  t.shape = shp;
  t.data.assign(data, data + (ndim ? n : 1));
  e->host[key] = std::move(t);
  e->finalized = false;
  return MMT_OK;
}

int mmt_finalize(mmt_engine* e) {
  if (!e) return MMT_E_ARG;
  std::string missing;
  for (auto& k : e->expected_order)
    if (!e->host.count(k)) missing += (missing.empty() ? "" : ", ") + k;
  if (!missing.empty()) return e->fail(MMT_E_WEIGHTS, "Missing key(s) in state_dict: " + missing);
  HIPCHECK(e, hipSetDevice(e->device));
  if (e->warena) {
    hipFree(e->warena);
    e->warena = nullptr;
    e->wused = 0;
  }
  drop_graphs(e);
  int r = pack_weights(e);
  if (r != MMT_OK) return r;
  e->host.clear();
  e->finalized = true;
  return MMT_OK;
}

// device frames are read in place: order the engine stream after the work queued so far on the
// caller's producer stream (e.g. the GPU frame assembly of mmt_rgbd_assemble / mmt_rgbx_merge)
static int wait_frame_stream(mmt_engine* e) {
  if (!e->frame_wait) return MMT_OK;
  // a caller stream with nothing left to run has already produced the frames: no event hop between the launches
  // (one sequence 1 124 -> 1 130 frames/s, 32 sequences level, profiles/r06_ab_frame_query.txt)
  if (hipStreamQuery(e->frame_stream) == hipSuccess) return MMT_OK;
  HIPCHECK(e, hipEventRecord(e->frame_ev, e->frame_stream));
  HIPCHECK(e, hipStreamWaitEvent(e->stream, e->frame_ev, 0));
  return MMT_OK;
}

int mmt_set_frame_stream(mmt_engine* e, void* hip_stream) {
  int r = check_engine(e);
  if (r) return r;
  e->frame_stream = (hipStream_t)hip_stream;
  e->frame_wait = true;
  return MMT_OK;
}

int mmt_initialize(mmt_engine* e, int slot, const uint8_t* frame, int Hh, int Ww, int Cc, int64_t row_stride,
                   int is_device, const double init_xywh[4]) {
  int r = check_engine(e);
  if (r) return r;
  if (slot < 0 || slot >= e->cfg.max_batch || !init_xywh) return e->fail(MMT_E_ARG, "bad slot / box");
  if (e->unfetched) return e->fail(MMT_E_STATE, "initialize with unfetched frames in flight");
  int x1, y1, cs;
  double rf;
  TRY(geometry(e, init_xywh, e->cfg.template_factor, e->cfg.template_size, &x1, &y1, &cs, &rf));
  const uint8_t* dev;
  if (is_device) TRY(wait_frame_stream(e));
  TRY(stage_frame(e, slot, 0, frame, Hh, Ww, Cc, row_stride, is_device, &dev, e->stream));
  const Acts v = act_view(e, slot, 0);   // the slot's template rows, launch row 0's parameters
  CropParam p{dev, row_stride, Hh, Ww, Cc, x1, y1, cs, 0};
  e->params_host[0] = p;
  HIPCHECK(e, hipMemcpyAsync(v.params_dev, e->params_host, sizeof(CropParam), hipMemcpyHostToDevice, e->stream));
  CropArgs ca{};
  ca.params = v.params_dev;
  ca.B = 1;
  ca.out_sz = e->cfg.template_size;
  ca.C = e->cfg.in_chans;
  ca.A_rgb = v.A_rgb;
  ca.A_aux = v.A_aux;
  ca.A_rgb_lo = v.A_rgb_l;
  ca.A_aux_lo = v.A_aux_l;
  ca.rows_per_seq = e->L;
  ca.row0 = 0;
  ca.dbg_patch = nullptr;
  crop_patchify(ca, e->stream);
  HIPCHECK(e, hipGetLastError());
  HIPCHECK(e, hipStreamSynchronize(e->stream));
  e->state[slot] = {init_xywh[0], init_xywh[1], init_xywh[2], init_xywh[3]};
  TRY(write_state(e, slot));
  e->active[slot] = 1;
  return MMT_OK;
}

int mmt_track_batch_submit(mmt_engine* e, int first_slot, int n, const uint8_t* const* frames, const int* Hs,
                           const int* Ws, int Cc, const int64_t* row_stride, int is_device, int64_t* ticket) {
  int r = check_engine(e);
  if (r) return r;
  if (n <= 0 || first_slot < 0 || first_slot + n > e->cfg.max_batch || !frames || !Hs || !Ws || !row_stride ||
      !ticket)
    return e->fail(MMT_E_ARG, "bad batch");
  auto& t = e->ring[e->next_ticket % kRing];
  if (t.open) return e->fail(MMT_E_STATE, "too many unfetched frames (fetch before submitting more)");
  if (e->probe && e->unfetched > 0) return e->fail(MMT_E_STATE, "the timing probe needs fetch before the next submit");
  const int entry = (int)(e->launches % kRing);   // the ring entry this launch's geometry / decode use
  CropParam* ph = e->params_host + (size_t)entry * e->cfg.max_batch;
  for (int i = 0; i < n; ++i) {
    const int slot = first_slot + i;
    if (!e->active[slot]) return e->fail(MMT_E_STATE, "track() before initialize() on slot " + std::to_string(slot));
    // with nothing in flight the host copy of the state is current: reject a bad box before any work
    // (the reference raises before touching its state); in flight, the device flags it per frame
    if (e->unfetched == 0) {
      int x1, y1, cs;
      double rf;
      TRY(geometry(e, e->state[slot].data(), e->cfg.search_factor, e->cfg.search_size, &x1, &y1, &cs, &rf));
    }
    const uint8_t* dev;
    TRY(stage_frame(e, slot, (int)(e->next_ticket % kRing), frames[i], Hs[i], Ws[i], Cc, row_stride[i], is_device,
                    &dev, e->cstream));
    ph[i] = CropParam{dev, row_stride[i], Hs[i], Ws[i], Cc, 0, 0, 0, 0};   // geometry: crop_geometry()
  }
  if (is_device) TRY(wait_frame_stream(e));
  if (!is_device) {   // the launch waits for this frame's copies only (copy stream, overlapping compute)
    hipEvent_t ce = e->copy_ev[e->next_ticket % kRing];
    HIPCHECK(e, hipEventRecord(ce, e->cstream));
    HIPCHECK(e, hipStreamWaitEvent(e->stream, ce, 0));
  }
  if (!e->ring_handoff)
    HIPCHECK(e, hipMemcpyAsync(e->acts.params_dev, ph, n * sizeof(CropParam), hipMemcpyHostToDevice, e->stream));
  const GraphEntry* replayed = nullptr;
  TRY(launch(e, first_slot, n, &replayed));
  if (!e->ring_handoff) {
    TrackOut* oh = e->outs_host + (size_t)entry * e->cfg.max_batch;
    HIPCHECK(e, hipMemcpyAsync(oh, e->acts.out_dev, (size_t)n * sizeof(TrackOut), hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHECK(e, hipEventRecord(t.done, e->stream));
  t.id = e->next_ticket++;
  t.first = first_slot;
  t.n = n;
  t.open = true;
  t.replayed = replayed;
  t.entry = entry;
  ++e->unfetched;
  *ticket = t.id;
  e->last_batch = n;
  return MMT_OK;
}

int mmt_track_batch_fetch(mmt_engine* e, int64_t ticket, double* out_xywh, float* out_score) {
  if (!e) return MMT_E_ARG;
  if (ticket < 0) return e->fail(MMT_E_ARG, "bad ticket");
  auto& t = e->ring[ticket % kRing];
  if (!t.open || t.id != ticket) return e->fail(MMT_E_ARG, "unknown or already fetched ticket");
  HIPCHECK(e, hipSetDevice(e->device));
  HIPCHECK(e, hipEventSynchronize(t.done));
  t.open = false;
  --e->unfetched;
  if (t.replayed)
    probe_collect_graph(e, *t.replayed);
  else
    probe_collect(e);
  const TrackOut* oh = e->outs_host + (size_t)t.entry * e->cfg.max_batch;
  int rc = MMT_OK;
  for (int i = 0; i < t.n; ++i) {
    const int slot = t.first + i;
    e->state[slot] = {oh[i].box[0], oh[i].box[1], oh[i].box[2], oh[i].box[3]};
    if (out_xywh)
      for (int k = 0; k < 4; ++k) out_xywh[4 * i + k] = oh[i].box[k];
    if (out_score) out_score[i] = oh[i].score;
    if (oh[i].err && rc == MMT_OK)
      rc = e->fail(oh[i].err, oh[i].err == MMT_E_BOX ? "Too small bounding box." : "crop size out of range");
  }
  return rc;
}

int mmt_track_batch(mmt_engine* e, int first_slot, int n, const uint8_t* const* frames, const int* Hs,
                    const int* Ws, int Cc, const int64_t* row_stride, int is_device, double* out_xywh,
                    float* out_score) {
  int64_t ticket;
  int r = mmt_track_batch_submit(e, first_slot, n, frames, Hs, Ws, Cc, row_stride, is_device, &ticket);
  if (r) return r;
  return mmt_track_batch_fetch(e, ticket, out_xywh, out_score);
}

int mmt_track(mmt_engine* e, int slot, const uint8_t* frame, int Hh, int Ww, int Cc, int64_t row_stride,
              int is_device, double out_xywh[4], float* out_score) {
  return mmt_track_batch(e, slot, 1, &frame, &Hh, &Ww, Cc, &row_stride, is_device, out_xywh, out_score);
}

int mmt_get_state(const mmt_engine* e, int slot, double out_xywh[4]) {
  if (!e || slot < 0 || slot >= e->cfg.max_batch || !out_xywh) return MMT_E_ARG;
  for (int k = 0; k < 4; ++k) out_xywh[k] = e->state[slot][k];
  return MMT_OK;
}

int mmt_set_state(mmt_engine* e, int slot, const double xywh[4]) {
  if (!e || slot < 0 || slot >= e->cfg.max_batch || !xywh) return MMT_E_ARG;
  if (e->unfetched) return e->fail(MMT_E_STATE, "set_state with unfetched frames in flight");
  e->state[slot] = {xywh[0], xywh[1], xywh[2], xywh[3]};
  return write_state(e, slot);
}

int mmt_set_ce_template_mask(mmt_engine* e, int slot, const uint8_t* mask, int n) {
  int r = check_engine(e);
  if (r) return r;
  if (!e->ce_mask) return e->fail(MMT_E_STATE, "engine not in mask mode (ce_template_index = MMT_CE_TEMPLATE_MASK)");
  if (!mask || n != e->Lz || slot < -1 || slot >= e->cfg.max_batch)
    return e->fail(MMT_E_ARG, "bad CE template mask (expect Lz bytes, slot in [-1, max_batch))");
  if (e->unfetched) return e->fail(MMT_E_STATE, "set_ce_template_mask with unfetched frames in flight");
  std::vector<int> rows(e->Lz, 0);
  int nr = 0;
  for (int i = 0; i < n; ++i)
    if (mask[i]) rows[nr++] = i;
  if (nr == 0) return e->fail(MMT_E_ARG, "CE template mask selects no token");
  // stream-ordered after the frames enqueued so far, synchronous (the host vectors die here), as write_state
  for (int sl = slot < 0 ? 0 : slot; sl < (slot < 0 ? e->cfg.max_batch : slot + 1); ++sl) {
    const Acts v = act_view(e, sl, 0);
    HIPCHECK(e, hipMemcpyAsync(v.ce_rows, rows.data(), (size_t)e->Lz * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(v.ce_nrows, &nr, 4, hipMemcpyHostToDevice, e->stream));
  }
  HIPCHECK(e, hipStreamSynchronize(e->stream));
  return MMT_OK;
}

int mmt_debug_fetch(mmt_engine* e, const char* what, int bi, void* dst, size_t nbytes) {
  int r = check_engine(e);
  if (r) return r;
  if (!e->cfg.debug_outputs) return e->fail(MMT_E_STATE, "engine built without debug_outputs");
  if (!what || !dst || bi < 0 || bi >= e->cfg.max_batch) return e->fail(MMT_E_ARG, "bad debug fetch");
  const Acts& a = e->acts;
  const std::string w(what);
  const std::pair<const char*, const void*> bufs[] = {{"crop", a.dbg_patch}, {"maps", a.dbg_maps},
                                                      {"feat", a.dbg_feat},  {"removed", a.removed},
                                                      {"result", a.res},     {"ce_keys", a.ce_keys}};
  const void* src = nullptr;
  for (auto& b : bufs)
    if (w == b.first) src = b.second;
  if (!src) return e->fail(MMT_E_ARG, "unknown debug buffer " + w);
  const size_t sz = act_bytes(e, src);   // of launch row bi (every buffer here is indexed by launch row)
  if (nbytes < sz) return e->fail(MMT_E_ARG, "debug buffer too small");
  HIPCHECK(e, hipMemcpy(dst, static_cast<const char*>(src) + bi * sz, sz, hipMemcpyDeviceToHost));
  return MMT_OK;
}

int mmt_debug_force_ce(mmt_engine* e, int slot, const float* keys, size_t n_floats) {
  int r = check_engine(e);
  if (r) return r;
  if (!e->cfg.debug_outputs) return e->fail(MMT_E_STATE, "engine built without debug_outputs");
  const size_t per = act_bytes(e, e->acts.ce_forced) / sizeof(float);
  if (e->unfetched) return e->fail(MMT_E_STATE, "force_ce with unfetched frames in flight");
  if (!keys) {
    e->force_ce = false;
  } else {
    if (slot < 0 || slot >= e->cfg.max_batch || n_floats != per) return e->fail(MMT_E_ARG, "bad forced CE keys");
    HIPCHECK(e, hipMemcpy(e->acts.ce_forced + (size_t)slot * per, keys, per * 4, hipMemcpyHostToDevice));
    e->force_ce = true;
  }
  drop_graphs(e);   // captured graphs carry the old kernel arguments
  return MMT_OK;
}

int mmt_timing_enable(mmt_engine* e, const char* cls) {
  if (!e) return MMT_E_ARG;
  if (!cls || !*cls) {
    if (e->probe)
      for (auto& p : e->probe->ev) {
        hipEventDestroy(p.first);
        hipEventDestroy(p.second);
      }
    e->probe.reset();
    return MMT_OK;
  }
  if (!e->probe) e->probe = std::make_unique<TimingProbe>();
  e->probe->cls = cls;
  e->probe->launches = 0;
  e->probe->total_ms = e->probe->flops = e->probe->bytes = 0;
  return MMT_OK;
}

int mmt_timing_read(mmt_engine* e, int* launches, double* total_ms, double* flops, double* bytes) {
  if (!e || !e->probe) return MMT_E_STATE;
  if (launches) *launches = (int)e->probe->launches;
  if (total_ms) *total_ms = e->probe->total_ms;
  if (flops) *flops = e->probe->flops;
  if (bytes) *bytes = e->probe->bytes;
  return MMT_OK;
}

}  // extern "C"
