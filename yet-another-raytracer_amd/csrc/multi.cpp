// multi.cpp — the multi-GPU half of the C ABI (include/yart.h): RCCL communicators, the frame
// gather, and yart_render_multi (one process driving N devices).
//
// Reference: the frame is 64 tile jobs fanned out over a thread pool and stitched back into one
// image from an mpsc channel (main.rs:633-660, 747-760). Here pixels are independent as there, so
// the devices share nothing while they render: 8x8 block b belongs to device b % N, each device
// renders its blocks straight into a packed buffer (its pixels and nothing else), and ONE gather
// over RCCL (point-to-point over xGMI: one hop per device, 1/N of the frame each) lands every
// packet on the root, where one kernel scatters them into the frame.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <system_error>
#include <thread>
#include <string>
#include <vector>

#include "../../include/yart.h"
#include "kernels.h"
#include "scene_impl.h"

using namespace yart_dev;
using namespace yart_impl;

struct yart_comm {
  ncclComm_t comm = nullptr;
  int device = 0, rank = 0, n_ranks = 1;
  DevBuf recv;  // root-side receive buffer (n_ranks packets), grown on demand
  ~yart_comm() {
    if (recv) { (void)hipSetDevice(device); (void)recv.release(); }
    if (comm) (void)ncclCommDestroy(comm);
  }
};

namespace {

int nccl_fail(ncclResult_t r, const char* what) {
  return fail(YART_ERR_DEVICE, std::string(what) + ": " + ncclGetErrorString(r));
}
#define NCCL_TRY(expr, what)                         \
  do {                                               \
    ncclResult_t r_ = (expr);                        \
    if (r_ != ncclSuccess) return nccl_fail(r_, what); \
  } while (0)

uint64_t packet_len(uint32_t w, uint32_t h, uint32_t n) {  // doubles per rank: the largest shard (shard 0)
  return yart_shard_packed_len(w, h, 0, n);
}

// The gather of one rank (inside a group for single-process communicators). Packets are equal
// sized (ncclGather's contract): a shard with fewer blocks sends the tail of its buffer too, which
// the unpack never reads. The send buffer must therefore hold packet_len doubles.
int enqueue_gather(yart_comm* c, const double* d_packed, uint32_t w, uint32_t h, int root, hipStream_t st) {
  const uint64_t n = packet_len(w, h, (uint32_t)c->n_ranks);
  // no stream to drain: the release of the old buffer waits for the device
  if (c->rank == root) HIP_TRY(c->recv.reserve(sizeof(double) * n * (size_t)c->n_ranks, {}), "hipMalloc gather buffer");
  NCCL_TRY(ncclGather(d_packed, c->rank == root ? c->recv.get<double>() : nullptr, n, ncclFloat64, root, c->comm, st),
           "ncclGather");
  return YART_OK;
}

}  // namespace

extern "C" {

int yart_comm_unique_id(uint8_t id_out[YART_COMM_ID_BYTES]) {
  if (!id_out) return fail(YART_ERR_INVALID, "null argument");
  static_assert(sizeof(ncclUniqueId) == YART_COMM_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId id;
  NCCL_TRY(ncclGetUniqueId(&id), "ncclGetUniqueId");
  std::memcpy(id_out, &id, sizeof id);
  return ok();
}

int yart_comm_init_rank(const uint8_t id[YART_COMM_ID_BYTES], int n_ranks, int rank, int device, yart_comm** out) {
  if (!id || !out || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(YART_ERR_INVALID, "bad argument");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
  if (device < 0 || device >= ndev) return fail(YART_ERR_INVALID, "device index out of range");
  DeviceGuard g(device);
  auto c = std::make_unique<yart_comm>();
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof uid);
  NCCL_TRY(ncclCommInitRank(&c->comm, n_ranks, uid, rank), "ncclCommInitRank");
  c->device = device; c->rank = rank; c->n_ranks = n_ranks;
  *out = c.release();
  return ok();
}

int yart_comm_init_all(int n, const int* devices, yart_comm** comms_out) {
  if (n < 1 || !devices || !comms_out) return fail(YART_ERR_INVALID, "bad argument");
  std::vector<ncclComm_t> comms((size_t)n, nullptr);
  NCCL_TRY(ncclCommInitAll(comms.data(), n, devices), "ncclCommInitAll");
  for (int d = 0; d < n; ++d) {
    comms_out[d] = new yart_comm();
    comms_out[d]->comm = comms[(size_t)d];
    comms_out[d]->device = devices[d]; comms_out[d]->rank = d; comms_out[d]->n_ranks = n;
  }
  return ok();
}

void yart_comm_destroy(yart_comm* c) { delete c; }

int yart_gather_frame_async(yart_comm* c, const double* d_packed, uint32_t w, uint32_t h, int root, double* d_frame,
                            void* stream) {
  if (!c || !d_packed || w == 0 || h == 0 || root < 0 || root >= c->n_ranks) return fail(YART_ERR_INVALID, "bad argument");
  if (c->rank == root && !d_frame) return fail(YART_ERR_INVALID, "null frame on the root");
  DeviceGuard g(c->device);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = enqueue_gather(c, d_packed, w, h, root, st)) return rc;
  if (c->rank == root)
    HIP_TRY(launch_unpack_shards(c->recv.get<double>(), (uint32_t)c->n_ranks, packet_len(w, h, (uint32_t)c->n_ranks), w, h,
                                 d_frame, st), "launch k_unpack_shards");
  return ok();
}

}  // extern "C"


// ------------------------------------------------------------ one process, N devices
// A slot is what the frames submitted on one caller stream use: a stream, a packed shard and a
// gather event per device, and the root's receive buffer. Frames on different caller streams
// overlap (the next frame's renders take the SIMD slots the previous frame's drain leaves idle);
// the gathers still run in submission order on every device (each waits for the previous
// submission's gather on its device), which is the order RCCL needs on a communicator.
struct SlotDevice {    // a slot's part on one device
  Stream stream;       // library-owned, non-blocking
  DevBuf packed;       // packet_len doubles
  Event gathered;      // its ncclGather of the latest frame
  Event rendered;      // its render of the latest frame (yart_multi_query)
  // its ncclGather's interval (from its launch, after its render and the previous submission's
  // gather, to its end) for each frame not yet read — the per-device balance of the first N-GPU
  // runs (which device waited in the gather for which)
  std::vector<EventPool::Lease> gather_events;
};
struct MultiSlot {
  std::vector<SlotDevice> dev;
  Event start;         // devices[0]: the caller stream's work before the frame
  Event done;          // devices[0]: the frame unpacked
  DevBuf recv;         // devices[0]: every shard's packet
  // devices[0]: the root's gather + unpack interval of each frame not yet read (timing)
  std::vector<EventPool::Lease> gather_events;
  uint64_t last_use = 0;  // submission number of its latest frame (eviction order)
};

struct yart_multi {
  int n = 0;
  std::vector<int> devices;
  std::vector<yart_scene*> scenes;
  std::vector<yart_comm*> comms;
  std::mutex mu;                                   // submissions are enqueued one at a time
  // recycled pairs of timing events, of devices[0] and per device (before the slots, whose leases
  // return into them)
  EventPool gather_pool;
  std::vector<EventPool> dev_pool;
  std::map<hipStream_t, std::unique_ptr<MultiSlot>> slots;  // by caller stream (devices[0]), at most kMaxSlots
  uint64_t submissions = 0;
  MultiSlot* latest = nullptr;  // the slot of the latest submission (yart_multi_query)
  std::vector<hipEvent_t> last_gather;             // per device: the latest submission's gather
  Stream host_stream;                              // devices[0]: yart_render_multi's caller stream
  DevBuf frame;                                    // devices[0]: yart_render_multi's frame
  double render_ms = 0.0, gather_ms = 0.0;  // yart_render_multi's last frame
  // per device, summed over the frames of the latest timing read (yart_multi_frame_timing or
  // yart_render_multi): render-kernel time and its own gather time (yart_multi_device_timing)
  std::vector<double> dev_render_ms, dev_gather_ms;
  uint32_t dev_frames = 0;
  // Drains a slot's streams and frees what it holds (the destructor; eviction of the least recently
  // used slot when a new caller stream would exceed kMaxSlots, so a caller that makes a stream per
  // frame does not grow device memory without bound — ADVICE r03).
  void release_slot(MultiSlot& s) {
    for (size_t d = 0; d < s.dev.size(); ++d) {
      (void)hipSetDevice(devices[d]);
      (void)hipStreamSynchronize(s.dev[d].stream);
    }
    // each device's part goes while that device is current, the last device first: devices[0] is
    // then current for the root's part, which goes with the rest of the slot
    while (!s.dev.empty()) {
      const size_t d = s.dev.size() - 1;
      (void)hipSetDevice(devices[d]);
      // the scene's unread frame-timing events of this stream: read and recycled now, or a later
      // stream that happens to get the same handle would report these frames as its own
      double r = 0.0, a = 0.0;
      uint32_t f = 0;
      (void)yart_frame_timing(scenes[d], s.dev[d].stream, &r, &a, &f);
      s.dev.pop_back();  // unread gather timings are dropped: their events return to the pools
    }
    s = MultiSlot{};
  }
  ~yart_multi() {
    for (auto& kv : slots) release_slot(*kv.second);
    for (size_t d = devices.size(); d-- > 0;) {  // devices[0] last: current for the root's members below
      (void)hipSetDevice(devices[d]);
      dev_pool[d].clear();
    }
    gather_pool.clear();
    (void)frame.release();
    if (host_stream) (void)hipStreamSynchronize(host_stream);
    host_stream.reset();
    for (yart_comm* c : comms) delete c;
    for (yart_scene* s : scenes) yart_scene_destroy(s);
  }
};

namespace {

struct RestoreDevice {
  int d = 0;
  RestoreDevice() { (void)hipGetDevice(&d); }
  ~RestoreDevice() { (void)hipSetDevice(d); }
};

// The slot of a caller stream, created on first use (streams and events made once, reused). At
// most kMaxSlots live at once: a new caller stream beyond that takes the place of the least
// recently used slot, after that slot's frames have finished (its streams are drained).
constexpr size_t kMaxSlots = 8;
int multi_slot(yart_multi* m, hipStream_t caller, MultiSlot** out) {
  auto it = m->slots.find(caller);
  if (it == m->slots.end()) {
    if (m->slots.size() >= kMaxSlots) {
      auto lru = m->slots.begin();
      for (auto i = m->slots.begin(); i != m->slots.end(); ++i)
        if (i->second->last_use < lru->second->last_use) lru = i;
      if (m->latest == lru->second.get()) m->latest = nullptr;
      m->release_slot(*lru->second);
      m->slots.erase(lru);
    }
    // built completely before it joins the map: a failure leaves no entry behind, and what was made
    // so far goes with `s`
    auto s = std::make_unique<MultiSlot>();
    s->dev.resize((size_t)m->n);
    for (int d = 0; d < m->n; ++d) {
      SlotDevice& D = s->dev[(size_t)d];
      HIP_TRY(hipSetDevice(m->devices[(size_t)d]), "hipSetDevice");
      HIP_TRY(D.stream.create(), "hipStreamCreate");
      HIP_TRY(D.gathered.create(), "hipEventCreate");
      HIP_TRY(D.rendered.create(), "hipEventCreate");
      if (d == 0) {
        HIP_TRY(s->start.create(), "hipEventCreate");
        HIP_TRY(s->done.create(), "hipEventCreate");
      }
    }
    it = m->slots.emplace(caller, std::move(s)).first;
  }
  it->second->last_use = ++m->submissions;
  *out = it->second.get();
  return YART_OK;
}

// Enqueue one frame: every device renders its shard into its packed buffer on the slot's stream,
// the grouped ncclGather follows each render in stream order, and devices[0] unpacks into
// d_frame after the caller stream's earlier work; the caller stream then waits for the frame.
// No host wait. prog: one progress word per device, or null.
int multi_submit(yart_multi* m, const yart_camera* cam, const yart_render_params* p, double* d_frame, hipStream_t caller,
                 std::vector<Progress>* prog) {
  if (!cam || !p || !d_frame) return fail(YART_ERR_INVALID, "null argument");
  if (p->width == 0 || p->height == 0) return fail(YART_ERR_INVALID, "width and height must be > 0");
  const int n = m->n;
  const uint32_t W = p->width, H = p->height;
  const uint64_t stride = packet_len(W, H, (uint32_t)n);
  const size_t pk_bytes = sizeof(double) * stride;
  RestoreDevice restore;
  MultiSlot* S = nullptr;
  if (int rc = multi_slot(m, caller, &S)) return rc;
  // the latest submission from here on, even one that fails partway (yart_multi_query then
  // describes it, not an older frame whose slot events this one is about to re-record)
  m->latest = S;
  // 1. renders, one per device, each straight into its packed shard. A wavefront (mesh) frame keeps
  // the host in its launch loop until the frame's last iterations are queued, so those devices are
  // driven from a host thread each, all at once.
  auto render_one = [&](int d) -> int {
    const size_t di = (size_t)d;
    HIP_TRY(hipSetDevice(m->devices[di]), "hipSetDevice");
    SlotDevice& D = S->dev[di];
    hipStream_t st = D.stream;
    if (D.packed.bytes() < pk_bytes) {
      HIP_TRY(D.packed.reserve(pk_bytes, {st}), "hipMalloc packed shard");
      // a smaller shard sends its tail too (equal-sized packets); zeroed once, never read
      HIP_TRY(hipMemsetAsync(D.packed.get<void>(), 0, pk_bytes, st), "hipMemset");
    }
    RenderArgs a;
    yart_render_params q = *p;
    q.shard_index = (uint32_t)d;
    q.shard_count = (uint32_t)n;
    if (int rc = make_args(m->scenes[di], cam, &q, D.packed.get<double>(), a)) return rc;
    a.packed = 1;
    Progress* pr = prog ? &(*prog)[di] : nullptr;
    if (int rc = launch_frame(m->scenes[di], a, p->samples_per_unit, false, st, pr)) return rc;
    HIP_TRY(hipEventRecord(D.rendered, st), "hipEventRecord");
    return YART_OK;
  };
  if (n > 1 && m->scenes[0]->wavefront) {
    std::vector<int> rcs((size_t)n, YART_OK);
    std::vector<std::string> errs((size_t)n);
    std::vector<std::thread> th;
    std::vector<int> here;
    for (int d = 1; d < n; ++d) {
      try {
        th.emplace_back([&, d] { rcs[(size_t)d] = render_one(d); errs[(size_t)d] = yart_last_error(); });
      } catch (const std::system_error&) {
        here.push_back(d);
      }
    }
    rcs[0] = render_one(0);
    errs[0] = yart_last_error();
    for (int d : here) { rcs[(size_t)d] = render_one(d); errs[(size_t)d] = yart_last_error(); }
    for (auto& t : th) t.join();
    for (int d = 0; d < n; ++d)
      if (rcs[(size_t)d] != YART_OK) return fail(rcs[(size_t)d], errs[(size_t)d]);  // the message was thread-local
  } else {
    for (int d = 0; d < n; ++d)
      if (int rc = render_one(d)) return rc;
  }
  // 2. the root's receive buffer (per slot: a later slot's gather may land while this one unpacks)
  HIP_TRY(hipSetDevice(m->devices[0]), "hipSetDevice");
  HIP_TRY(S->recv.reserve(pk_bytes * (size_t)n, {S->dev[0].stream}), "hipMalloc gather buffer");
  // The frame's timing pairs are leases until both ends are recorded and join the slot's lists
  // only then (below): a submission that fails half way returns them to their pools instead of
  // leaving a pair that multi_timing cannot read.
  EventPool::Lease gev;
  HIP_TRY(m->gather_pool.take(2, gev), "hipEventCreate");
  std::vector<EventPool::Lease> dev_ev((size_t)n);
  // 3. ONE gather to devices[0], each device's part right behind its render; in submission order
  for (int d = 0; d < n; ++d) {
    const size_t di = (size_t)d;
    SlotDevice& D = S->dev[di];
    HIP_TRY(hipSetDevice(m->devices[di]), "hipSetDevice");
    if (m->last_gather[di] && m->last_gather[di] != D.gathered)
      HIP_TRY(hipStreamWaitEvent(D.stream, m->last_gather[di], 0), "hipStreamWaitEvent");
    if (d == 0) HIP_TRY(hipEventRecord(gev[0], D.stream), "hipEventRecord");
    HIP_TRY(m->dev_pool[di].take(2, dev_ev[di]), "hipEventCreate");
    HIP_TRY(hipEventRecord(dev_ev[di][0], D.stream), "hipEventRecord");
  }
  NCCL_TRY(ncclGroupStart(), "ncclGroupStart");
  for (int d = 0; d < n; ++d) {
    const size_t di = (size_t)d;
    (void)hipSetDevice(m->devices[di]);
    ncclResult_t r = ncclGather(S->dev[di].packed.get<double>(), d == 0 ? S->recv.get<double>() : nullptr, stride,
                                ncclFloat64, 0, m->comms[di]->comm, S->dev[di].stream);
    if (r != ncclSuccess) { (void)ncclGroupEnd(); return nccl_fail(r, "ncclGather"); }
  }
  NCCL_TRY(ncclGroupEnd(), "ncclGroupEnd");
  for (int d = 0; d < n; ++d) {
    const size_t di = (size_t)d;
    SlotDevice& D = S->dev[di];
    HIP_TRY(hipSetDevice(m->devices[di]), "hipSetDevice");
    HIP_TRY(hipEventRecord(dev_ev[di][1], D.stream), "hipEventRecord");
    HIP_TRY(hipEventRecord(D.gathered, D.stream), "hipEventRecord");
    m->last_gather[di] = D.gathered;
  }
  // 4. unpack on the root, after whatever the caller stream had queued (it may still read d_frame)
  const hipStream_t root = S->dev[0].stream;
  HIP_TRY(hipSetDevice(m->devices[0]), "hipSetDevice");
  HIP_TRY(hipEventRecord(S->start, caller), "hipEventRecord");
  HIP_TRY(hipStreamWaitEvent(root, S->start, 0), "hipStreamWaitEvent");
  HIP_TRY(launch_unpack_shards(S->recv.get<double>(), (uint32_t)n, stride, W, H, d_frame, root), "launch k_unpack_shards");
  HIP_TRY(hipEventRecord(gev[1], root), "hipEventRecord");
  S->gather_events.push_back(std::move(gev));  // both ends recorded: handed over
  for (int d = 0; d < n; ++d) S->dev[(size_t)d].gather_events.push_back(std::move(dev_ev[(size_t)d]));
  HIP_TRY(hipEventRecord(S->done, root), "hipEventRecord");
  HIP_TRY(hipStreamWaitEvent(caller, S->done, 0), "hipStreamWaitEvent");
  return YART_OK;
}

// The summed intervals of a slot's timing pairs (on the current device). The pairs are taken out of
// the slot first and recycled whatever happens: a failed read does not leave pairs behind for every
// later call to trip over.
hipError_t sum_pairs(std::vector<EventPool::Lease>& pairs, double& sum) {
  std::vector<EventPool::Lease> evs;
  evs.swap(pairs);
  hipError_t bad = hipSuccess;
  for (auto& e : evs) {
    float ms = 0.0f;
    if (bad == hipSuccess && (bad = hipEventElapsedTime(&ms, e[0], e[1])) == hipSuccess) sum += ms;
  }
  return bad;
}

// Summed kernel times of the frames submitted since the last read, over every slot or one
// (their streams idle by then): render = the slowest device's summed k_render time,
// gather = the root's gather + unpack intervals, which include the root's wait for the slowest
// device's render to finish. Per device (m->dev_*): its summed render time and the summed
// intervals of its own ncclGather.
int multi_timing(yart_multi* m, MultiSlot* only, double* render_ms, double* gather_ms, uint32_t* frames) {
  RestoreDevice restore;
  double worst = 0.0;
  uint32_t nf = 0;
  m->dev_render_ms.assign((size_t)m->n, 0.0);
  m->dev_gather_ms.assign((size_t)m->n, 0.0);
  for (int d = 0; d < m->n; ++d) {
    double r = 0.0, dg = 0.0;
    for (auto& kv : m->slots) {
      if (only && kv.second.get() != only) continue;
      SlotDevice& D = kv.second->dev[(size_t)d];
      double rr = 0.0, acc = 0.0;
      uint32_t f = 0;
      if (int rc = yart_frame_timing(m->scenes[(size_t)d], D.stream, &rr, &acc, &f)) return rc;
      r += rr;
      if (d == 0) nf += f;
      HIP_TRY(hipSetDevice(m->devices[(size_t)d]), "hipSetDevice");
      HIP_TRY(sum_pairs(D.gather_events, dg), "hipEventElapsedTime");
    }
    m->dev_render_ms[(size_t)d] = r;
    m->dev_gather_ms[(size_t)d] = dg;
    if (r > worst) worst = r;
  }
  m->dev_frames = nf;
  HIP_TRY(hipSetDevice(m->devices[0]), "hipSetDevice");
  double g = 0.0;
  for (auto& kv : m->slots)
    if (!only || kv.second.get() == only) HIP_TRY(sum_pairs(kv.second->gather_events, g), "hipEventElapsedTime");
  *render_ms = worst;
  *gather_ms = g;
  *frames = nf;
  return YART_OK;
}

}  // namespace

extern "C" {

int yart_multi_create(int n, const int* devices, const yart_scene_desc* desc, yart_multi** out) {
  if (n < 1 || !devices || !desc || !out) return fail(YART_ERR_INVALID, "bad argument");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
  for (int d = 0; d < n; ++d) {
    if (devices[d] < 0 || devices[d] >= ndev) return fail(YART_ERR_INVALID, "device index out of range");
    for (int e = 0; e < d; ++e)
      if (devices[e] == devices[d]) return fail(YART_ERR_INVALID, "a device listed twice");
  }
  auto m = std::make_unique<yart_multi>();
  m->n = n;
  m->devices.assign(devices, devices + n);
  m->last_gather.assign((size_t)n, nullptr);
  m->dev_pool = std::vector<EventPool>((size_t)n);
  RestoreDevice restore;
  for (int d = 0; d < n; ++d) {  // the scene is uploaded once per device, here
    yart_scene* s = nullptr;
    if (int rc = yart_scene_create(devices[d], desc, &s)) return rc;
    m->scenes.push_back(s);
  }
  HIP_TRY(hipSetDevice(devices[0]), "hipSetDevice");
  HIP_TRY(m->host_stream.create(), "hipStreamCreate");
  m->comms.assign((size_t)n, nullptr);
  if (int rc = yart_comm_init_all(n, devices, m->comms.data())) return rc;
  *out = m.release();
  return ok();
}

int yart_render_multi_async(yart_multi* m, const yart_camera* cam, const yart_render_params* p, double* d_frame,
                            void* stream) {
  if (!m) return fail(YART_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(m->mu);
  if (int rc = multi_submit(m, cam, p, d_frame, (hipStream_t)stream, nullptr)) return rc;
  return ok();
}

int yart_multi_frame_timing(yart_multi* m, double* render_ms, double* gather_ms, uint32_t* frames) {
  if (!m || !render_ms || !gather_ms || !frames) return fail(YART_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(m->mu);
  if (int rc = multi_timing(m, nullptr, render_ms, gather_ms, frames)) return rc;
  return ok();
}

int yart_render_multi(yart_multi* m, const yart_camera* cam, const yart_render_params* p, double* xyz_sum_out,
                      yart_progress_fn progress, void* user) {
  if (!m || !cam || !p || !xyz_sum_out) return fail(YART_ERR_INVALID, "null argument");
  if (p->width == 0 || p->height == 0) return fail(YART_ERR_INVALID, "width and height must be > 0");
  std::lock_guard<std::mutex> lk(m->mu);
  const int n = m->n;
  const size_t frame_bytes = sizeof(double) * 3 * (size_t)p->width * p->height;
  RestoreDevice restore;
  HIP_TRY(hipSetDevice(m->devices[0]), "hipSetDevice");
  hipStream_t hs = m->host_stream;
  HIP_TRY(m->frame.reserve(frame_bytes, {hs}), "hipMalloc frame");
  double* d_frame = m->frame.get<double>();
  std::vector<Progress> pr((size_t)(progress ? n : 0));
  uint64_t total_px = 0;
  std::vector<Progress*> pp;
  for (int d = 0; d < (int)pr.size(); ++d) {
    HIP_TRY(hipSetDevice(m->devices[(size_t)d]), "hipSetDevice");
    if (int rc = alloc_progress(pr[(size_t)d])) return rc;
    pr[(size_t)d].pixels = shard_pixels(p->width, p->height, (uint32_t)d, (uint32_t)n);
    total_px += pr[(size_t)d].pixels;
    pp.push_back(&pr[(size_t)d]);
  }
  // everything (renders, gather, unpack) is enqueued before the host waits
  if (int rc = multi_submit(m, cam, p, d_frame, hs, progress ? &pr : nullptr)) return rc;
  HIP_TRY(hipSetDevice(m->devices[0]), "hipSetDevice");
  Event done;
  HIP_TRY(done.create(), "hipEventCreate");
  HIP_TRY(hipEventRecord(done, hs), "hipEventRecord");
  if (int rc = wait_with_progress({done}, {m->devices[0]}, pp, total_px, progress, user)) return rc;
  HIP_TRY(hipSetDevice(m->devices[0]), "hipSetDevice");
  HIP_TRY(hipMemcpyAsync(xyz_sum_out, d_frame, frame_bytes, hipMemcpyDeviceToHost, hs), "copy frame");
  HIP_TRY(hipStreamSynchronize(hs), "copy frame");
  uint32_t frames = 0;
  // the host stream's slot is idle now: the timing of its frame
  double r = 0.0, g = 0.0;
  if (int rc = multi_timing(m, m->latest, &r, &g, &frames)) return rc;
  m->render_ms = frames ? r / frames : 0.0;
  m->gather_ms = frames ? g / frames : 0.0;
  return ok();
}

int yart_multi_last_timing(const yart_multi* m, double* render_ms, double* gather_ms) {
  if (!m || !render_ms || !gather_ms) return fail(YART_ERR_INVALID, "null argument");
  *render_ms = m->render_ms;
  *gather_ms = m->gather_ms;
  return ok();
}

int yart_multi_device_timing(yart_multi* m, int n, double* render_ms, double* gather_ms, uint32_t* frames) {
  if (!m || !render_ms || !gather_ms || !frames) return fail(YART_ERR_INVALID, "null argument");
  if (n != m->n) return fail(YART_ERR_INVALID, "n must be the multi's device count");
  std::lock_guard<std::mutex> lk(m->mu);
  for (int d = 0; d < n; ++d) {
    render_ms[d] = (size_t)d < m->dev_render_ms.size() ? m->dev_render_ms[(size_t)d] : 0.0;
    gather_ms[d] = (size_t)d < m->dev_gather_ms.size() ? m->dev_gather_ms[(size_t)d] : 0.0;
  }
  *frames = m->dev_frames;
  return ok();
}

int yart_multi_query(yart_multi* m, int32_t* state, int32_t* unpacked) {
  if (!m || !state || !unpacked) return fail(YART_ERR_INVALID, "null argument");
  // never waits: a submission in progress (its thread may be blocked in the gather's setup) holds the
  // lock, and then every device reads -1
  std::unique_lock<std::mutex> lk(m->mu, std::try_to_lock);
  *unpacked = -1;
  for (int d = 0; d < m->n; ++d) state[d] = -1;
  if (!lk.owns_lock() || !m->latest) return ok();
  RestoreDevice restore;
  MultiSlot& S = *m->latest;
  auto done = [](hipEvent_t e) { return e && hipEventQuery(e) == hipSuccess; };
  for (int d = 0; d < m->n; ++d) {
    (void)hipSetDevice(m->devices[(size_t)d]);
    state[d] = done(S.dev[(size_t)d].gathered) ? 2 : done(S.dev[(size_t)d].rendered) ? 1 : 0;
  }
  (void)hipSetDevice(m->devices[0]);
  *unpacked = done(S.done) ? 1 : 0;
  return ok();
}

void yart_multi_destroy(yart_multi* m) { delete m; }

int yart_unpack_shards_async(int device, const double* d_recv, uint32_t shards, uint64_t stride, uint32_t width,
                             uint32_t height, double* d_frame, void* stream) {
  if (!d_recv || !d_frame || shards == 0 || width == 0 || height == 0) return fail(YART_ERR_INVALID, "bad argument");
  if (stride < packet_len(width, height, shards)) return fail(YART_ERR_INVALID, "stride below the largest shard's packet");
  DeviceGuard g(device);
  HIP_TRY(launch_unpack_shards(d_recv, shards, stride, width, height, d_frame, (hipStream_t)stream), "launch k_unpack_shards");
  return ok();
}

}  // extern "C"
