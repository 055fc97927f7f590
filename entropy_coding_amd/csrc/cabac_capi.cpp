// C ABI of libcabac_hip.so (declared in include/cabac_hip.h).  Host-side plumbing only: argument
// checks, stream/event handling, and the host-pointer entry points' path over PCIe: pinned host memory
// (cabac_hip_host_alloc / _register) is DMA'd directly, pageable memory goes through a ring of pinned bounce
// blocks, a batch is cut into chunks whose H2D copy, kernel and D2H copy run on separate streams, and coded
// substreams leave the device compacted (cabac_assemble.hip) in one copy per chunk.  There is no
// CPU codec in this library — without a GPU cabac_hip_init fails.
//
// How the file is laid out: the slot table (every device staging buffer of a ctx, by name) and the ctx; the helpers every
// section uses (fail / ensure, the event brackets Bracket, TIMED_LAUNCH and Timed, the PCIe path, the level / link checks and the
// WPP and rows schedules); then one section per header.  The single-launch device calls go through TIMED_LAUNCH.  The four
// host-pointer forms of the parser family (residual, unit, element and plan parse, the rows parse included) share their host
// checks (check_substream_host, check_plan_host, check_coeff_ranges_host) and their staging (ParseStage), the family's device calls
// their operands (cabac::ParseIn) and their prelude (parse_device_call); the device pipelines of the plan write share their
// tables and the one wait (plan_write_tables, wait_for_totals).  Every other host-pointer form but the chunked codec pipeline stages
// through Stage (a slot, the copy, the typed pointer; plain or through the bounce ring) and shares what it has in common with another:
// stage_rows, CandStage, PayloadReturn, check_records_host, flags_status; the device pipelines take operand structs (SpliceIn,
// cabac::PlanWriteIn, PayloadOut).  The pipelined forms keep their own stream choreography.  The blocking runtime calls go through counting helpers (wait_stream,
// device_alloc, ...: cabac_hip_workspace_waits); on a ctx with a fixed workspace (cabac_hip_workspace.h) the three pipelines that wait
// in the middle take a branch that queues a gate kernel instead.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "cabac_hip.h"
#include "cabac_hip_ctx_sets.h"
#include "cabac_hip_pieces.h"
#include "cabac_hip_piece_encoder.h"
#include "cabac_hip_estimate.h"
#include "cabac_hip_nal.h"
#include "cabac_hip_parse_elements.h"
#include "cabac_hip_parse_plan.h"
#include "cabac_hip_parse_unit.h"
#include "cabac_hip_plan_rows.h"
#include "cabac_hip_plan_continue.h"
#include "cabac_hip_plan_resume.h"
#include "cabac_hip_probe.h"
#include "cabac_hip_rec10.h"
#include "cabac_hip_search.h"
#include "cabac_hip_search_emit.h"
#include "cabac_hip_search_plan.h"
#include "cabac_hip_search_unit.h"
#include "cabac_hip_sparse.h"
#include "cabac_hip_splice_rows.h"
#include "cabac_hip_workspace.h"
#include "cabac_hip_write_plan.h"
#include "cabac_kernels.h"
#include "cabac_nal_kernels.h"
#include "cabac_rec10_kernels.h"
#include "cabac_sparse_kernels.h"

#ifdef CABAC_PARSE_PROFILE
namespace cabac {
hipError_t debug_read_parse_prof(unsigned long long *out);
hipError_t debug_read_parse_waves(unsigned long long *out);
}
#endif

// Every device staging buffer of a ctx (index into d_buf / d_cap; grown on demand by ensure), in numeric order.  Names of one
// value side by side: one buffer in two roles, in calls that never overlap.
enum Slot {
  // the codec's host-pointer forms (encode, decode, estimate, NAL and WPP batch), cabac_hip_residual_batch, the parser family
  kDesc = 0,                                          // substream descriptors | residual_batch: block descriptors
  kRecords = 1, kCoeff = 1,                           // bin records | parser family, residual_batch: coefficients
  kBytes = 2, kOutRecords = 2,                        // byte slots | residual_batch: the records
  kResults = 3, kFracBits = 3, kRecOffsets = 3, kFirstTus = 3,  // results | estimate_batch | residual_batch | parsers: tile_first, pad, tus
  kBins = 4, kFlags = 4, kCounts = 4, kParseResults = 4,        // decoded bins | estimate_batch | residual_batch: counts, info | parsers
  kResidualScratch = 5,                               // the residual binariser's scratch (every call that runs it)
  kPayload = 6, kPackedBins = 6, kTuInfo = 6,         // compacted payload | decode_batch_packed | parsers: info words
  kPayloadOffsets = 7,
  // the spliced-residual path (also the plan write and the plan resolve), the staging of its host-pointer form (also the plan write's)
  kSpCnt = 8, kSpPlan = 9, kSpDesc = 10, kSpTuOff = 11, kSpRec = 12, kSpBytes = 13, kSpFlag = 14,
  kSpInDesc = 15, kSpInRec = 16, kSpInFirst = 17, kSpInSplice = 18, kSpInTu = 19, kSpInCoeff = 20, kSpOutRes = 21, kSpOutInfo = 22,
  kSpOutCnt = 23,
  // the fused residual estimator: the candidate order, the staging of its host-pointer form (also the search rounds')
  kEstScratch = 24, kEstInFirst = 25, kEstInTu = 26, kEstInCoeff = 27, kEstInState = 28, kEstInRate = 29, kEstInSet = 30,
  kEstOutBits = 31, kEstOutInfo = 32,
  // emulation prevention: the chunk summaries and scans, the staging of the host-pointer forms
  kNalScratch = 33, kNalIn = 34, kNalInOff = 35, kNalOut = 36, kNalOutOff = 37, kNalLoc = 38, kNalStatus = 39,
  // the search rounds' host-pointer forms (the side records of cabac_hip_search_unit.h included; the plan round's resolved form)
  kSearchInGroupFirst = 40, kSearchInOutSet = 41, kSearchInDist = 42, kSearchOutPick = 43, kSearchOutCost = 44, kSearchInRecords = 45,
  kSearchInRecFirst = 46, kSearchInTuAt = 47,
  // the winner log's emit
  kLogScratch = 48, kLogDesc = 49, kLogFirst = 50, kLogRec = 51, kLogSplice = 52,
  // the unit parse: runs, positions (also the element / plan parse, the plan write, the plan round), side bins
  kUnitRecords = 53, kUnitTuAt = 54, kUnitBins = 55,
  // the element and plan parse: plan, block guards, values (also the plan write and the plan round)
  kElemPlan = 56, kElemGuard = 57, kElemValues = 58,
  // the plan write: its per-substream words, the descriptor list of its records pass (also the plan round's resolved blocks)
  kPwPlan = 59, kPwTu = 60,
  // the plan resolve of the search rounds: counts (and flags where the caller gives none), staged ent_first, flags
  kPsCnt = 61, kPsEnt = 62, kPsFlags = 63,
  // a WPP call (the rows parse shares the sets): one set per substream, prefix descriptors, checked links and slot indices, the
  // results of the prefix passes, and the links of every host-pointer form with rows
  kWppState = 64, kWppRate = 65, kWppDesc = 66, kWppIndex = 67, kWppRes = 68, kWppFrom = 69, kWppAt = 70,
  // the plan rows and the spliced rows: per substream the record index of its hand-over entry, then the out sets of the substreams
  // that did not stop (the rows write); the hand-over splice counts of the spliced rows' host-pointer form
  kRowsWords = 71, kSpInSync = 72,
  // the sparse coefficient transport (cabac_hip_sparse.h): the error words and workgroup counts of its kernels, and the firsts,
  // entries and status of its host-pointer forms
  kSparseScratch = 73, kSparseFirst = 74, kSparseEnt = 75, kSparseStatus = 76,
  // the packed bin records (cabac_hip_rec10.h): the blocks of the host-pointer forms as they came up, unpacked into kRecords
  kRec10 = 77,
  // probe points (cabac_hip_probe.h): the probes of a spliced call as positions in the expanded strings; the lists, the splice
  // counts and the values of the host-pointer forms (which stage the rest as the estimator's and the spliced call's forms do)
  kProbeRec = 78, kProbeFirst = 79, kProbeAt = 80, kProbeSplice = 81, kProbeOut = 82,
  kSlots
};

struct cabac_hip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  bool timed = false;
  int enc_variant = 0, dec_variant = 0;
  int piece_encoder = 4;  // cabac_hip_piece_encoder.h: the encoder of the pieces calls (4, 7, 0 = by the batch)
  std::string last_error;
  // per-launch profiling ring (cabac_hip_profile_enable)
  std::vector<hipEvent_t> prof_ev;  // 2 per slot
  std::vector<int32_t> prof_kind;
  uint32_t prof_n = 0;
  // device staging (the Slot table above)
  void *d_buf[kSlots] = {};
  size_t d_cap[kSlots] = {};
  void *h_totals = nullptr;  // pinned, 64 bytes: what the spliced-residual path reads back in the middle
  uint32_t *d_select = nullptr;  // kMaxChunks + 1 device words: the decode dispatch's on-device choice, one per launch in flight
  // ---- the PCIe path of the host-pointer entry points -------------------------------------------------
  static constexpr int kKernelStreams = 4, kMaxChunks = 8, kBounceDepth = 4;
  static constexpr size_t kBounceBlock = size_t(4) << 20;
  hipStream_t s_in = nullptr, s_out = nullptr, s_k[kKernelStreams] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_in[kMaxChunks] = {}, ev_k[kMaxChunks] = {}, ev_out[kMaxChunks] = {};
  struct Bounce {  // ring of pinned blocks between pageable caller memory and the DMA engines
    void *blk[kBounceDepth] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev[kBounceDepth] = {nullptr, nullptr, nullptr, nullptr};
    bool busy[kBounceDepth] = {false, false, false, false};
    void *dst[kBounceDepth] = {nullptr, nullptr, nullptr, nullptr};  // D2H: where the block goes once it has arrived
    size_t len[kBounceDepth] = {0, 0, 0, 0};
    int next = 0;
  } bounce_in, bounce_out;
  void *h_pin[2] = {nullptr, nullptr};  // pinned: [0] results + payload offsets coming back, [1] compacted payload
  size_t h_cap[2] = {0, 0};
  bool pipe_ready = false;
  int chunks_override = 0;  // CABAC_HIP_CHUNKS (experiments); 0 = by batch size
  std::vector<cabac_search_log *> logs;  // the winner logs that are alive (cabac_hip_search_emit.h): destroyed with the ctx
  // ---- the fixed workspace (cabac_hip_workspace.h) -----------------------------------------------------
  uint64_t n_waits = 0;               // blocking runtime calls issued for this ctx (the helpers below count them)
  bool ws_fixed = false;
  cabac_workspace_sizes ws = {};      // what the workspace was fixed to
  cabac::WsState *d_ws = nullptr;     // its device words (allocated by the first fix, kept)
  cabac_workspace_status ws_last = {0, 0, 0, 0, 0, CABAC_WS_NONE_VOIDED};  // the status as the last release found it
};

// a winner log: fixed device arrays (one allocation each, never grown) and the ctx whose stream orders everything done to them
struct cabac_search_log {
  cabac_hip_ctx *ctx = nullptr;
  cabac::SearchLogArrays a = {};
  int coeff_bytes = 4;
};

namespace {

int fail_hip(cabac_hip_ctx *c, hipError_t e, const char *what) {
  if (c) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    c->last_error = buf;
  }
  return CABAC_HIP_ERR_HIP;
}

int fail(cabac_hip_ctx *c, int status, const char *what) {
  if (c) c->last_error = what;
  return status;
}

#define HIP_TRY(c, expr)                                   \
  do {                                                     \
    hipError_t _e = (expr);                                \
    if (_e != hipSuccess) return fail_hip((c), _e, #expr); \
  } while (0)

// The blocking runtime calls of this file, counted for cabac_hip_workspace_waits where they are issued (c may be null).
hipError_t wait_stream(cabac_hip_ctx *c, hipStream_t st) {
  if (c) c->n_waits++;
  return hipStreamSynchronize(st);
}
hipError_t wait_event(cabac_hip_ctx *c, hipEvent_t ev) {
  if (c) c->n_waits++;
  return hipEventSynchronize(ev);
}
template <class T>
hipError_t device_alloc(cabac_hip_ctx *c, T **p, size_t bytes) {
  if (c) c->n_waits++;
  return hipMalloc(reinterpret_cast<void **>(p), bytes);
}
hipError_t device_free(cabac_hip_ctx *c, void *p) {
  if (c) c->n_waits++;
  return hipFree(p);
}
hipError_t pinned_alloc(cabac_hip_ctx *c, void **p, size_t bytes, unsigned flags) {
  if (c) c->n_waits++;
  return hipHostMalloc(p, bytes, flags);
}
hipError_t pinned_free(cabac_hip_ctx *c, void *p) {
  if (c) c->n_waits++;
  return hipHostFree(p);
}

int ensure(cabac_hip_ctx *c, int slot, size_t bytes) {
  if (bytes == 0) bytes = 16;
  if (c->d_cap[slot] >= bytes) return CABAC_HIP_OK;
  if (c->d_buf[slot]) {
    HIP_TRY(c, device_free(c, c->d_buf[slot]));
    c->d_buf[slot] = nullptr;
    c->d_cap[slot] = 0;
  }
  size_t want = bytes + bytes / 4 + 256;
  hipError_t e = device_alloc(c, &c->d_buf[slot], want);
  if (e != hipSuccess) {
    c->last_error = "hipMalloc failed";
    return CABAC_HIP_ERR_NOMEM;
  }
  c->d_cap[slot] = want;
  return CABAC_HIP_OK;
}

// a plain copy on the ctx stream, host to device and back (nothing for no bytes); the pipelined forms use h2d / d2h below
hipError_t up(cabac_hip_ctx *c, void *dst, const void *src, size_t n) {
  return n ? hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, c->stream) : hipSuccess;
}
hipError_t down(cabac_hip_ctx *c, void *dst, const void *src, size_t n) {
  return n ? hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
}

// Event bracket of one launch: the ring slot when profiling is on, else the ctx's single pair.
struct Bracket {
  hipEvent_t a, b;
};
Bracket bracket_for(cabac_hip_ctx *c, int kind) {
  if (!c->prof_ev.empty() && c->prof_n < c->prof_kind.size()) {
    uint32_t i = c->prof_n++;
    c->prof_kind[i] = kind;
    return {c->prof_ev[2 * i], c->prof_ev[2 * i + 1]};
  }
  return {c->ev_start, c->ev_stop};
}

// One launch on the ctx stream between the events of its bracket; cabac_hip_last_kernel_ms reads the ctx's pair, so it has a time
// only when the ring did not take the launch.  what: the launch as last_error names it when it fails.
template <class F>
int timed_launch(cabac_hip_ctx *c, int kind, const char *what, F &&launch) {
  Bracket br = bracket_for(c, kind);
  HIP_TRY(c, hipEventRecord(br.a, c->stream));
  if (hipError_t e = launch(); e != hipSuccess) return fail_hip(c, e, what);
  HIP_TRY(c, hipEventRecord(br.b, c->stream));
  c->timed = (br.a == c->ev_start);
  return CABAC_HIP_OK;
}
#define TIMED_LAUNCH(c, kind, expr) timed_launch((c), (kind), #expr, [&] { return (expr); })

struct Timed {  // profile-ring bracket around a group of launches (nothing when the ring is off or full)
  cabac_hip_ctx *c;
  Bracket br{nullptr, nullptr};
  Timed(cabac_hip_ctx *ctx, int kind) : c(ctx) {
    if (!c->prof_ev.empty() && c->prof_n < c->prof_kind.size()) {
      br = bracket_for(c, kind);
      (void)hipEventRecord(br.a, c->stream);
    }
  }
  ~Timed() {
    if (br.b) (void)hipEventRecord(br.b, c->stream);
  }
};

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

int check_desc_host(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, uint64_t n_records_total,
                    uint64_t bytes_total) {
  for (uint32_t s = 0; s < n_sub; s++) {
    const cabac_substream_desc &d = desc[s];
    if (d.rec_offset > n_records_total || d.n_records > n_records_total - d.rec_offset)
      return fail(c, CABAC_HIP_ERR_INVALID, "records out of range");
    if (d.byte_offset > bytes_total || d.byte_capacity > bytes_total - d.byte_offset)
      return fail(c, CABAC_HIP_ERR_INVALID, "bytes out of range");
    if (d.byte_offset & 15u) return fail(c, CABAC_HIP_ERR_INVALID, "byte_offset must be 16-byte aligned");
    if ((d.init_id & 3u) > 2u) return fail(c, CABAC_HIP_ERR_INVALID, "init_id must be 0..2");
  }
  return CABAC_HIP_OK;
}

// What a form that takes bin records and no byte ranges refuses about substream s: its record range, its init_id, then `more` (the
// form's own finding about s, or null).  named: the message begins "substream s: " (the rows form of the spliced call), else it is bare
int check_records_host(cabac_hip_ctx *c, uint32_t s, const cabac_substream_desc &d, uint64_t n_records_total, const char *more = nullptr,
                       bool named = false) {
  const char *what = more;
  if (d.rec_offset > n_records_total || d.n_records > n_records_total - d.rec_offset) what = "records out of range";
  else if ((d.init_id & 3u) > 2u) what = "init_id must be 0..2";
  if (!what) return CABAC_HIP_OK;
  char buf[96];
  snprintf(buf, sizeof buf, "substream %u: %s", s, what);
  return fail(c, CABAC_HIP_ERR_INVALID, named ? buf : what);
}

// The flags (or results) a call fetched, to the caller's array where there is one (out null, or got itself: nothing to copy); any of
// them set: CABAC_HIP_ERR_SUBSTREAM and the form's message.  status: what the form has found so far
inline uint32_t flag_of(uint32_t f) { return f; }
inline uint32_t flag_of(const cabac_substream_result &r) { return r.flags; }
template <class T>
int flags_status(cabac_hip_ctx *c, uint32_t n, const T *got, T *out, const char *message, int status = CABAC_HIP_OK) {
  for (uint32_t i = 0; i < n; i++) {
    if (out && out != got) out[i] = got[i];
    if (flag_of(got[i])) status = CABAC_HIP_ERR_SUBSTREAM;
  }
  if (status) c->last_error = message;
  return status;
}

// ---- the host checks of the parser family's host-pointer forms, in the order every form runs them: per substream the three
// checks below and then the form's own, and behind all substreams the blocks' coefficient ranges -------------------------------
// bytes_total: null where the descriptors' byte ranges are not input (the plan write, the plan round)
int check_substream_host(cabac_hip_ctx *c, const cabac_substream_desc &d, const uint32_t *tile_first, uint32_t s, const uint64_t *bytes_total) {
  if (tile_first[s] > tile_first[s + 1]) return fail(c, CABAC_HIP_ERR_INVALID, "tile_first must not decrease");
  if (bytes_total && (d.byte_offset > *bytes_total || d.byte_capacity > *bytes_total - d.byte_offset))
    return fail(c, CABAC_HIP_ERR_INVALID, "bytes out of range");
  if ((d.init_id & 3u) > 2u) return fail(c, CABAC_HIP_ERR_INVALID, "init_id must be 0..2");
  return CABAC_HIP_OK;
}

int check_coeff_ranges_host(cabac_hip_ctx *c, uint32_t n_tu, const cabac_tu_desc *tus, uint64_t n_coeff_total) {
  for (uint32_t t = 0; t < n_tu; t++) {
    if (tus[t].log2_width > 6 || tus[t].log2_height > 6) continue;  // flagged by the kernel, writes nothing
    const uint64_t n = uint64_t(1) << (tus[t].log2_width + tus[t].log2_height);
    if (tus[t].coeff_offset > n_coeff_total || n > n_coeff_total - tus[t].coeff_offset)
      return fail(c, CABAC_HIP_ERR_INVALID, "coefficients out of range");
  }
  return CABAC_HIP_OK;
}

// ---- pinned host memory handed out by cabac_hip_host_alloc / pinned in place by cabac_hip_host_register ----
std::mutex g_host_mu;
std::unordered_map<const void *, size_t> g_host_owned, g_host_registered;

bool host_is_pinned(const void *p, size_t bytes) {
  if (!p) return false;
  {
    std::lock_guard<std::mutex> lk(g_host_mu);
    for (const auto *m : {&g_host_owned, &g_host_registered})
      for (const auto &kv : *m) {
        const uint8_t *b = static_cast<const uint8_t *>(kv.first), *q = static_cast<const uint8_t *>(p);
        if (q >= b && q + bytes <= b + kv.second) return true;
      }
  }
  // pinned by somebody else (e.g. torch's pin_memory): the first AND the last byte must be host memory the runtime knows, inside
  // ONE allocation whose extent the runtime can tell — a range that starts in a pinned allocation and runs past its end, or
  // whose end cannot be established, is treated as pageable (it then goes through the bounce ring, which is always safe)
  const uint8_t *q = static_cast<const uint8_t *>(p);
  hipPointerAttribute_t a, z;
  if (hipPointerGetAttributes(&a, q) != hipSuccess || hipPointerGetAttributes(&z, q + (bytes ? bytes - 1 : 0)) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (a.type != hipMemoryTypeHost || z.type != hipMemoryTypeHost) return false;
  hipDeviceptr_t base = nullptr;
  size_t extent = 0;
  if (hipMemGetAddressRange(&base, &extent, const_cast<uint8_t *>(q)) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  const uint8_t *b = static_cast<const uint8_t *>(base);
  return q >= b && q + bytes <= b + extent;
}

// Nothing of the ctx's own streams is in flight afterwards and no bounce block is waiting to be handed over: the state a
// host-pointer call must leave behind when it returns early (the blocks' destinations point into the caller's buffers,
// which the caller may free as soon as the call has returned — they are dropped, not copied).
void pipe_quiesce(cabac_hip_ctx *c) {
  (void)wait_stream(c, c->stream);  // null = the adopted default stream: synchronised like any other
  for (hipStream_t st : {c->s_in, c->s_out, c->s_k[0], c->s_k[1], c->s_k[2], c->s_k[3]})
    if (st) (void)wait_stream(c, st);
  for (cabac_hip_ctx::Bounce *b : {&c->bounce_in, &c->bounce_out})
    for (int i = 0; i < cabac_hip_ctx::kBounceDepth; i++) {
      b->busy[i] = false;
      b->dst[i] = nullptr;
      b->len[i] = 0;
    }
}

// the exit of every host-pointer entry point: an error other than "a substream has a flag set" may have come from the middle
// of the pipeline.  The contract of such a return ("payload_capacity too small" is the one a caller meets
// in ordinary use): the outputs' contents are unspecified, the library does not write to caller memory on behalf of the call once
// it has returned, and the ctx is usable as before.  Only error paths wait here: a call that returns CABAC_HIP_OK never does.
int host_call_exit(cabac_hip_ctx *c, int rc) {
  if (c && c->pipe_ready && rc != CABAC_HIP_OK && rc != CABAC_HIP_ERR_SUBSTREAM) {
    const std::string keep = c->last_error;
    DeviceGuard g(c->device);
    pipe_quiesce(c);
    (void)hipGetLastError();
    c->last_error = keep;
  }
  return rc;
}

void pipe_destroy(cabac_hip_ctx *c) {
  pipe_quiesce(c);
  for (hipStream_t st : {c->s_in, c->s_out, c->s_k[0], c->s_k[1], c->s_k[2], c->s_k[3]})
    if (st) (void)hipStreamDestroy(st);
  for (int i = 0; i < cabac_hip_ctx::kMaxChunks; i++)
    for (hipEvent_t e : {c->ev_in[i], c->ev_k[i], c->ev_out[i]})
      if (e) (void)hipEventDestroy(e);
  for (cabac_hip_ctx::Bounce *b : {&c->bounce_in, &c->bounce_out})
    for (int i = 0; i < cabac_hip_ctx::kBounceDepth; i++) {
      if (b->blk[i]) (void)pinned_free(c, b->blk[i]);
      if (b->ev[i]) (void)hipEventDestroy(b->ev[i]);
    }
  for (void *p : c->h_pin)
    if (p) (void)pinned_free(c, p);
  c->pipe_ready = false;
}

int pipe_init(cabac_hip_ctx *c) {
  if (c->pipe_ready) return CABAC_HIP_OK;
  HIP_TRY(c, hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking));
  HIP_TRY(c, hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking));
  for (hipStream_t &st : c->s_k) HIP_TRY(c, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  for (int i = 0; i < cabac_hip_ctx::kMaxChunks; i++) {
    HIP_TRY(c, hipEventCreateWithFlags(&c->ev_in[i], hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&c->ev_k[i], hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&c->ev_out[i], hipEventDisableTiming));
  }
  for (cabac_hip_ctx::Bounce *b : {&c->bounce_in, &c->bounce_out})
    for (int i = 0; i < cabac_hip_ctx::kBounceDepth; i++) {
      HIP_TRY(c, pinned_alloc(c, &b->blk[i], cabac_hip_ctx::kBounceBlock, hipHostMallocDefault));
      HIP_TRY(c, hipEventCreateWithFlags(&b->ev[i], hipEventDisableTiming));
    }
  if (const char *e = getenv("CABAC_HIP_CHUNKS")) c->chunks_override = atoi(e);
  c->pipe_ready = true;
  return CABAC_HIP_OK;
}

int ensure_pinned(cabac_hip_ctx *c, int slot, size_t bytes) {
  if (bytes == 0) bytes = 16;
  if (c->h_cap[slot] >= bytes) return CABAC_HIP_OK;
  if (c->h_pin[slot]) {
    HIP_TRY(c, pinned_free(c, c->h_pin[slot]));
    c->h_pin[slot] = nullptr;
    c->h_cap[slot] = 0;
  }
  const size_t want = bytes + bytes / 4 + 4096;
  if (pinned_alloc(c, &c->h_pin[slot], want, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    c->last_error = "hipHostMalloc failed";
    return CABAC_HIP_ERR_NOMEM;
  }
  c->h_cap[slot] = want;
  return CABAC_HIP_OK;
}

// grow pinned slot `slot` to `bytes`, keeping its first `keep` bytes (copies into them may still be in flight on s_out)
int ensure_pinned_keep(cabac_hip_ctx *c, int slot, size_t bytes, size_t keep) {
  if (c->h_cap[slot] >= bytes && c->h_pin[slot]) return CABAC_HIP_OK;
  void *old = c->h_pin[slot];
  if (old && keep) HIP_TRY(c, wait_stream(c, c->s_out));
  c->h_pin[slot] = nullptr;
  c->h_cap[slot] = 0;
  int rc = ensure_pinned(c, slot, bytes + bytes);  // chunks are about equal: leave room for the ones to come
  if (rc == CABAC_HIP_OK && old && keep) std::memcpy(c->h_pin[slot], old, keep);
  if (old) (void)pinned_free(c, old);
  return rc;
}

// host -> device on `st`: pinned memory is DMA'd where it lies; pageable memory is copied block by block into the
// pinned ring, each block's DMA overlapping the host copy of the next one
int h2d(cabac_hip_ctx *c, void *dst, const void *src, size_t bytes, hipStream_t st) {
  if (bytes == 0) return CABAC_HIP_OK;
  if (host_is_pinned(src, bytes)) {
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
    return CABAC_HIP_OK;
  }
  cabac_hip_ctx::Bounce &b = c->bounce_in;
  for (size_t off = 0; off < bytes; off += cabac_hip_ctx::kBounceBlock) {
    const size_t n = std::min(cabac_hip_ctx::kBounceBlock, bytes - off);
    const int i = b.next;
    b.next = (i + 1) % cabac_hip_ctx::kBounceDepth;
    if (b.busy[i]) HIP_TRY(c, wait_event(c, b.ev[i]));
    std::memcpy(b.blk[i], static_cast<const uint8_t *>(src) + off, n);
    HIP_TRY(c, hipMemcpyAsync(static_cast<uint8_t *>(dst) + off, b.blk[i], n, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(b.ev[i], st));
    b.busy[i] = true;
  }
  return CABAC_HIP_OK;
}

// one block of the outgoing ring has arrived: hand it to the caller's memory
int d2h_retire(cabac_hip_ctx *c, int i) {
  cabac_hip_ctx::Bounce &b = c->bounce_out;
  if (!b.busy[i]) return CABAC_HIP_OK;
  HIP_TRY(c, wait_event(c, b.ev[i]));
  std::memcpy(b.dst[i], b.blk[i], b.len[i]);
  b.busy[i] = false;
  return CABAC_HIP_OK;
}

// device -> host on `st`; for pageable memory the data is complete only after d2h_drain
int d2h(cabac_hip_ctx *c, void *dst, const void *src, size_t bytes, hipStream_t st) {
  if (bytes == 0) return CABAC_HIP_OK;
  if (host_is_pinned(dst, bytes)) {
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    return CABAC_HIP_OK;
  }
  cabac_hip_ctx::Bounce &b = c->bounce_out;
  for (size_t off = 0; off < bytes; off += cabac_hip_ctx::kBounceBlock) {
    const size_t n = std::min(cabac_hip_ctx::kBounceBlock, bytes - off);
    const int i = b.next;
    b.next = (i + 1) % cabac_hip_ctx::kBounceDepth;
    if (int rc = d2h_retire(c, i)) return rc;
    HIP_TRY(c, hipMemcpyAsync(b.blk[i], static_cast<const uint8_t *>(src) + off, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipEventRecord(b.ev[i], st));
    b.busy[i] = true;
    b.dst[i] = static_cast<uint8_t *>(dst) + off;
    b.len[i] = n;
  }
  return CABAC_HIP_OK;
}

int d2h_drain(cabac_hip_ctx *c) {
  for (int k = 0; k < cabac_hip_ctx::kBounceDepth; k++) {
    const int i = (c->bounce_out.next + k) % cabac_hip_ctx::kBounceDepth;  // oldest first
    if (int rc = d2h_retire(c, i)) return rc;
  }
  return CABAC_HIP_OK;
}

// ---- the staging of every host-pointer form but the chunked codec pipeline (encode_batch_impl / decode_batch_impl, which moves
// pieces of its arrays on several streams): room for `count` elements of T in a slot, the caller's array copied into it, the typed
// device pointer back.  Two transports: the plain copy on the ctx stream (up), or with `ring` h2d on `st` (pinned memory DMA'd where
// it lies, pageable memory through the bounce ring).  The first failure sticks: every later call does nothing and returns null, so
// a form stages all it needs in the order the copies are to run and asks once (rc).
struct Stage {
  cabac_hip_ctx *c;
  bool ring = false;
  hipStream_t st = nullptr;
  int rc = CABAC_HIP_OK;

  // room bytes in the slot; n of them from src where there is something to copy (n 0: nothing is issued)
  void *bytes(int slot, size_t room, const void *src, size_t n) {
    if (rc || (rc = ensure(c, slot, room))) return nullptr;
    void *d = c->d_buf[slot];
    if (ring) rc = h2d(c, d, src, n, st);
    else if (hipError_t e = up(c, d, src, n); e != hipSuccess) rc = fail_hip(c, e, "up(c, d, src, n)");
    return rc ? nullptr : d;
  }
  // room for count + pad elements, the first count of them from src
  template <class T>
  T *put(int slot, size_t count, const T *src, size_t pad = 0) {
    return static_cast<T *>(bytes(slot, (count + pad) * sizeof(T), src, count * sizeof(T)));
  }
  template <class T>
  T *room(int slot, size_t count) { return static_cast<T *>(bytes(slot, count * sizeof(T), nullptr, 0)); }
  // an array the caller may leave out: the slot all the same, a null pointer for the kernels
  template <class T>
  T *opt(int slot, size_t count, const T *src) {
    T *d = src ? put(slot, count, src) : room<T>(slot, count);
    return src ? d : nullptr;
  }
};

// What every payload-producing device pipeline writes (the spliced encode, the plan write, the log's emit): the compacted payload,
// its offsets, the results, and the blocks' info words (may be null)
struct PayloadOut {
  uint8_t *d_payload;
  uint64_t payload_capacity;
  uint64_t *d_payload_offsets;
  cabac_substream_result *d_results;
  uint32_t *d_tu_info;
};

// What the spliced encode reads: side records per substream and the blocks spliced into them
struct SpliceIn {
  const cabac_substream_desc *d_desc;
  const uint16_t *d_records;
  const uint32_t *d_splice_first;
  const cabac_splice *d_splices;
  uint32_t n_splice, n_tu;
  const cabac_tu_desc *d_tu;
  const void *d_coeff;
  int coeff_bytes;
};

// The way back of the two pipelined writer forms (the spliced encode, the plan write): results and offsets come back through the
// pinned block h_pin[0] on the ctx stream, behind them one word the form may add; the payload follows on s_out once its size is
// known.  prepare() before the uploads, fetch() behind the device pipeline (then the form's own d2h copies on s_out), finish() last.
struct PayloadReturn {
  cabac_hip_ctx *c;
  uint32_t n_sub;
  uint8_t *payload;
  uint64_t payload_capacity;
  uint64_t *payload_offsets;
  cabac_substream_result *results;
  PayloadOut d{};
  cabac_substream_result *h_res = nullptr;
  uint64_t *h_off = nullptr;
  uint32_t *h_word = nullptr;

  size_t res_bytes() const { return size_t(n_sub) * sizeof(cabac_substream_result); }
  size_t off_bytes() const { return (size_t(n_sub) + 1) * sizeof(uint64_t); }

  // the device side (d_tu_info: room for n_info words) and the pinned block
  int prepare(Stage &st, size_t n_info) {
    d = {st.room<uint8_t>(kPayload, payload_capacity ? payload_capacity : 16), payload_capacity,
         st.room<uint64_t>(kPayloadOffsets, size_t(n_sub) + 1), st.room<cabac_substream_result>(kSpOutRes, n_sub),
         st.room<uint32_t>(kSpOutInfo, n_info ? n_info : 1)};
    if (st.rc) return st.rc;
    if (int rc = ensure_pinned(c, 0, res_bytes() + off_bytes() + 64)) return rc;
    h_res = static_cast<cabac_substream_result *>(c->h_pin[0]);
    h_off = reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(c->h_pin[0]) + res_bytes());
    h_word = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(h_off) + off_bytes());
    return CABAC_HIP_OK;
  }

  // d_word (may be null): a device word that comes back with the results, into *h_word.  Waits for them, refuses a payload that does
  // not fit, queues the payload's copy
  int fetch(const uint32_t *d_word) {
    HIP_TRY(c, hipMemcpyAsync(h_res, d.d_results, res_bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_off, d.d_payload_offsets, off_bytes(), hipMemcpyDeviceToHost, c->stream));
    if (d_word) HIP_TRY(c, hipMemcpyAsync(h_word, d_word, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_k[1], c->stream));
    // the big things leave on the outgoing copy stream once the offsets are known
    HIP_TRY(c, wait_event(c, c->ev_k[1]));
    if (h_off[n_sub] > payload_capacity) return fail(c, CABAC_HIP_ERR_INVALID, "payload_capacity too small");
    return d2h(c, payload, d.d_payload, h_off[n_sub], c->s_out);
  }

  // everything queued on s_out has arrived; results and offsets to the caller; the flags (and what the form found: status) as the status
  int finish(int status, const char *message) {
    if (int rc = d2h_drain(c)) return rc;
    HIP_TRY(c, wait_stream(c, c->s_out));
    payload_offsets[0] = 0;
    for (uint32_t s = 0; s < n_sub; s++) payload_offsets[s + 1] = h_off[s + 1];
    return flags_status(c, n_sub, h_res, results, message, status);
  }
};

// A batch cut at substream boundaries into chunks of about equal record counts.  Chunks need the substreams' record
// and byte slots in ascending, non-overlapping order (what every packer produces); otherwise the batch is one chunk.
struct Chunk {
  uint32_t s0, s1;
  uint64_t rec_lo, rec_hi, byte_lo, byte_hi;
};

std::vector<Chunk> plan_chunks(const cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc) {
  uint64_t rec_end = 0, byte_end = 0, total = 0;
  bool ordered = true;
  for (uint32_t s = 0; s < n_sub; s++) {
    ordered = ordered && desc[s].rec_offset >= rec_end && desc[s].byte_offset >= byte_end;
    rec_end = std::max<uint64_t>(rec_end, desc[s].rec_offset + desc[s].n_records);
    byte_end = std::max<uint64_t>(byte_end, desc[s].byte_offset + desc[s].byte_capacity);
    total += desc[s].n_records;
  }
  // The kernels' time does not shrink below ~1 024 substreams (it is the length of the serial chains), and kernels of
  // different chunks were measured to run one after the other even on separate streams, so a batch of c chunks costs about
  // copy / c + c x kernel + tail: with the C4 batch (2.35 ms of H2D at 57 GB/s, 0.9 ms of kernel) two chunks are the
  // minimum (measured: 1 chunk 4.26 ms, 2 chunks 4.08, 4 chunks 4.86, 8 chunks 6.4).  Default: two chunks from 2 048
  // substreams and 16 M records up, else one; CABAC_HIP_CHUNKS overrides.
  int want = c->chunks_override > 0 ? c->chunks_override : (n_sub >= 2048u && (total >> 24) != 0u ? 2 : 1);
  want = std::max(1, std::min(want, (int)cabac_hip_ctx::kMaxChunks));
  if (!ordered || (uint32_t)want > n_sub) want = 1;
  std::vector<Chunk> out;
  uint32_t s = 0;
  uint64_t done = 0;
  for (int k = 0; k < want; k++) {
    Chunk ch;
    ch.s0 = s;
    const uint64_t goal = total * uint64_t(k + 1) / uint64_t(want);
    while (s < n_sub && (done < goal || k == want - 1)) done += desc[s++].n_records;
    if (k == want - 1) s = n_sub;
    ch.s1 = s;
    if (ch.s1 == ch.s0) continue;
    ch.rec_lo = ch.byte_lo = ~0ull;
    ch.rec_hi = ch.byte_hi = 0;
    for (uint32_t q = ch.s0; q < ch.s1; q++) {
      ch.rec_lo = std::min<uint64_t>(ch.rec_lo, desc[q].rec_offset);
      ch.rec_hi = std::max<uint64_t>(ch.rec_hi, desc[q].rec_offset + desc[q].n_records);
      ch.byte_lo = std::min<uint64_t>(ch.byte_lo, desc[q].byte_offset);
      ch.byte_hi = std::max<uint64_t>(ch.byte_hi, desc[q].byte_offset + desc[q].byte_capacity);
    }
    out.push_back(ch);
  }
  return out;
}

// The records of one chunk on their way to d_rec (kRecords).  16-bit records go up as they are.  Packed records (cabac_hip_rec10.h)
// go up as the whole blocks that hold [rec_lo, rec_hi), into kRec10 at the offset they have in the caller's buffer; a block that
// two chunks share goes up with both.  The unpack below then runs on the chunk's kernel stream, behind the chunk's ev_in and in
// front of its encode or decode launch, and writes [rec_lo, rec_hi) alone.
int upload_chunk_records(cabac_hip_ctx *c, const Chunk &ch, const void *records, bool rec10, uint16_t *d_rec) {
  if (!rec10)
    return h2d(c, d_rec + ch.rec_lo, static_cast<const uint16_t *>(records) + ch.rec_lo, (ch.rec_hi - ch.rec_lo) * 2, c->s_in);
  if (ch.rec_hi == ch.rec_lo) return CABAC_HIP_OK;
  const uint64_t lo = ch.rec_lo / CABAC_REC10_BLOCK_RECORDS * CABAC_REC10_BLOCK_BYTES, hi = CABAC_REC10_BYTES(ch.rec_hi);
  return h2d(c, static_cast<uint8_t *>(c->d_buf[kRec10]) + lo, static_cast<const uint8_t *>(records) + lo, hi - lo, c->s_in);
}

int unpack_chunk_records(cabac_hip_ctx *c, const Chunk &ch, hipStream_t ks, uint16_t *d_rec) {
  const bool ring = !c->prof_ev.empty() && c->prof_n < c->prof_kind.size();
  Bracket br = ring ? bracket_for(c, 43) : Bracket{nullptr, nullptr};
  if (ring) HIP_TRY(c, hipEventRecord(br.a, ks));
  HIP_TRY(c, cabac::launch_rec10_unpack(ks, static_cast<const uint8_t *>(c->d_buf[kRec10]), ch.rec_lo, ch.rec_hi - ch.rec_lo, d_rec));
  if (ring) HIP_TRY(c, hipEventRecord(br.b, ks));
  return CABAC_HIP_OK;
}

// ---- levels, links and context sets: what the WPP calls (cabac_hip_ctx_sets.h), the plan rows and the spliced rows share ------
// level_first as the WPP calls need it: n_level + 1 entries, non-decreasing, from 0 to n_sub
int check_levels(cabac_hip_ctx *c, uint32_t n_sub, uint32_t n_level, const uint32_t *level_first) {
  if (n_sub == 0) return CABAC_HIP_OK;
  if (n_level == 0 || !level_first || level_first[0] != 0u || level_first[n_level] != n_sub)
    return fail(c, CABAC_HIP_ERR_INVALID, "level_first must run from 0 to n_sub");
  for (uint32_t l = 0; l < n_level; l++)
    if (level_first[l] > level_first[l + 1]) {
      char buf[96];
      snprintf(buf, sizeof buf, "level_first decreases at level %u", l + 1);
      return fail(c, CABAC_HIP_ERR_INVALID, buf);
    }
  return CABAC_HIP_OK;
}

// the links of a host-pointer form (level_first checked): every link points into an earlier level
int check_links_host(cabac_hip_ctx *c, uint32_t n_sub, uint32_t n_level, const uint32_t *level_first, const uint32_t *sync_from) {
  for (uint32_t l = 0; l < n_level; l++)
    for (uint32_t s = level_first[l]; s < level_first[l + 1]; s++) {
      const uint32_t from = sync_from[s];
      if (from == CABAC_CTX_NO_SET || from < level_first[l]) continue;
      char buf[128];
      if (from >= n_sub) snprintf(buf, sizeof buf, "substream %u links to %u, beyond the batch", s, from);
      else snprintf(buf, sizeof buf, "substream %u (level %u) links to %u in the same or a later level", s, l, from);
      return fail(c, CABAC_HIP_ERR_INVALID, buf);
    }
  return CABAC_HIP_OK;
}

// the rows of a call of cabac_hip_plan_rows.h or cabac_hip_splice_rows.h: levels (HOST memory), links and hand-over positions
// (device memory; host memory in the batch forms).  d_sync_splice: the spliced rows' alone, and null there too where every block at
// the hand-over position goes in front
struct Rows {
  uint32_t n_level;
  const uint32_t *level_first, *d_sync_from, *d_sync_at, *d_sync_splice;
};

// the probes of a spliced call (cabac_hip_probe.h): the lists (device memory; host memory in the batch form; splice may be null)
// and where the values go
struct SpliceProbes {
  const uint32_t *first, *at, *splice;
  uint32_t n;
  uint32_t *bits;
};

// what the host-pointer forms of cabac_hip_probe.h refuse about a probe list (host memory)
int check_probes_host(cabac_hip_ctx *c, uint32_t n_sub, const uint32_t *probe_first, const uint32_t *probe_at, uint32_t n_probe) {
  if (n_sub == 0) return CABAC_HIP_OK;
  if (!probe_first || (n_probe && !probe_at)) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (probe_first[0] != 0) return fail(c, CABAC_HIP_ERR_INVALID, "probe_first must start at 0");
  for (uint32_t s = 0; s < n_sub; s++) {
    const char *what = nullptr;
    if (probe_first[s] > probe_first[s + 1]) what = "probe_first must not decrease";
    else if (probe_first[s + 1] > n_probe) what = "probe_first ends behind n_probe";
    else
      for (uint32_t p = probe_first[s] + 1; p < probe_first[s + 1] && !what; p++)
        if (probe_at[p] < probe_at[p - 1]) what = "probe positions go backwards";
    if (what) {
      char buf[96];
      snprintf(buf, sizeof buf, "substream %u: %s", s, what);
      return fail(c, CABAC_HIP_ERR_INVALID, buf);
    }
  }
  return CABAC_HIP_OK;
}

// what a host-pointer form refuses about its rows (links in host memory)
int check_rows_host(cabac_hip_ctx *c, uint32_t n_sub, const Rows &rows) {
  if (int bad = check_levels(c, n_sub, rows.n_level, rows.level_first)) return bad;
  return check_links_host(c, n_sub, rows.n_level, rows.level_first, rows.d_sync_from);
}

// the rows of a host-pointer form, staged: links and hand-over positions on the device, the levels where they are.  spliced: the form
// of cabac_hip_splice_rows.h, which has a slot for the hand-over splice counts (the caller may still leave them out)
Rows stage_rows(Stage &st, uint32_t n_sub, const Rows &rows, bool spliced) {
  const uint32_t *from = st.put(kWppFrom, n_sub, rows.d_sync_from), *at = st.put(kWppAt, n_sub, rows.d_sync_at);
  return Rows{rows.n_level, rows.level_first, from, at, spliced ? st.opt(kSpInSync, n_sub, rows.d_sync_splice) : nullptr};
}

// what a call on a fixed workspace (cabac_hip_workspace.h) may not exceed; checked before anything is queued.  (n_splice needs no
// check of its own: the splice pipeline has refused n_splice != n_tu by then.  cabac_workspace_sizes.n_entries sizes nothing.)
int check_workspace(cabac_hip_ctx *c, uint32_t n_sub, uint32_t n_tu, bool rows) {
  if (n_sub > c->ws.n_sub) return fail(c, CABAC_HIP_ERR_INVALID, "n_sub exceeds the fixed workspace");
  if (n_tu > c->ws.n_tu) return fail(c, CABAC_HIP_ERR_INVALID, "n_tu exceeds the fixed workspace");
  if (rows && !(c->ws.flags & CABAC_WS_ROWS)) return fail(c, CABAC_HIP_ERR_INVALID, "a rows call on a workspace fixed without CABAC_WS_ROWS");
  return CABAC_HIP_OK;
}
int refuse_fixed_batch(cabac_hip_ctx *c) {
  return fail(c, CABAC_HIP_ERR_INVALID,
              "the workspace is fixed: the host-pointer forms of this pipeline share its buffers; call cabac_hip_workspace_release first");
}

bool sets_args_ok(uint32_t n_sub, uint32_t n_sets, const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set,
                  const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate) {
  if (n_sub == 0) return true;
  if (d_start_set && n_sets && (!d_state || !d_rate)) return false;
  if (d_out_set && n_sets && (!d_out_state || !d_out_rate)) return false;
  return true;
}

// The schedule of a WPP call on the ctx stream: per level the level kernel (prefix descriptors, checked links, slot indices), for
// every level but the last its prefix pass into the slots, then the pass over all substreams from their slots.  encode: d_bins
// null, the prefix pass is the context advance; decode: the sets decoder (its bins land in d_bins and are written again, the
// same, by the last pass; its results go to a scratch).
int wpp_device_impl(cabac_hip_ctx *c, bool decode, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                    uint8_t *d_bytes, uint8_t *d_bins, cabac_substream_result *d_results, uint32_t n_level,
                    const uint32_t *level_first, const uint32_t *d_sync_from, const uint32_t *d_sync_at) {
  if (!c || (n_sub && (!d_desc || !d_records || !d_bytes || !d_results || (decode && !d_bins) || !d_sync_from || !d_sync_at)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (n_sub == 0) return CABAC_HIP_OK;
  int rc = check_levels(c, n_sub, n_level, level_first);
  if (rc) return rc;
  DeviceGuard g(c->device);
  const size_t set_words = size_t(n_sub) * CABAC_NUM_CONTEXTS;
  if ((rc = ensure(c, kWppState, set_words * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, kWppRate, set_words))) return rc;
  if ((rc = ensure(c, kWppDesc, size_t(n_sub) * sizeof(cabac_substream_desc)))) return rc;
  if ((rc = ensure(c, kWppIndex, 2 * size_t(n_sub) * sizeof(uint32_t)))) return rc;
  if (decode && (rc = ensure(c, kWppRes, size_t(n_sub) * sizeof(cabac_substream_result)))) return rc;
  auto *slot_state = static_cast<uint32_t *>(c->d_buf[kWppState]);
  auto *slot_rate = static_cast<uint8_t *>(c->d_buf[kWppRate]);
  auto *pre_desc = static_cast<cabac_substream_desc *>(c->d_buf[kWppDesc]);
  auto *start = static_cast<uint32_t *>(c->d_buf[kWppIndex]);
  auto *slot = start + n_sub;
  auto *pre_res = static_cast<cabac_substream_result *>(c->d_buf[kWppRes]);
  for (uint32_t l = 0; l < n_level; l++) {
    const uint32_t first = level_first[l], n = level_first[l + 1] - first;
    if (n == 0) continue;
    HIP_TRY(c, cabac::launch_wpp_level(c->stream, first, n, d_desc, d_sync_from, d_sync_at, pre_desc, start, slot));
    if (l + 1 == n_level) break;
    const cabac::CtxSets sets{n_sub, slot_state, slot_rate, start + first, slot + first, slot_state, slot_rate};
    Timed t(c, 33);
    if (decode)
      HIP_TRY(c, cabac::launch_decode(c->stream, c->dec_variant, n, pre_desc + first, d_records, d_bytes, d_bins, pre_res + first, 0,
                                      c->d_select, &sets));
    else
      HIP_TRY(c, cabac::launch_ctx_advance(c->stream, n, pre_desc + first, d_records, sets, nullptr));
  }
  const cabac::CtxSets sets{n_sub, slot_state, slot_rate, start, nullptr, nullptr, nullptr};
  Bracket br = bracket_for(c, decode ? 31 : 30);
  HIP_TRY(c, hipEventRecord(br.a, c->stream));
  if (decode)
    HIP_TRY(c, cabac::launch_decode(c->stream, c->dec_variant, n_sub, d_desc, d_records, d_bytes, d_bins, d_results, 0, c->d_select, &sets));
  else
    HIP_TRY(c, cabac::launch_encode(c->stream, c->enc_variant, n_sub, d_desc, d_records, d_bytes, d_results, 0, &sets));
  HIP_TRY(c, hipEventRecord(br.b, c->stream));
  c->timed = (br.a == c->ev_start);
  return CABAC_HIP_OK;
}

// The schedule of a rows parse on the ctx stream: for every non-empty level ONE launch of the sets kernel over that level's
// substreams.  A substream starts from the slot of its link (checked on the device against the level: it must lie below the
// level's first substream) and writes its own slot at its hand-over entry; the last level writes none.
int parse_rows_device_impl(cabac_hip_ctx *c, uint32_t n_sub, const cabac::ParseIn &in, const Rows &rows) {
  if (!c || (n_sub && (!in.desc || !in.bytes || !in.tile_first || !in.results || !rows.d_sync_from || !rows.d_sync_at)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (in.coeff_bytes != 4 && in.coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (n_sub == 0) return CABAC_HIP_OK;
  int rc = check_levels(c, n_sub, rows.n_level, rows.level_first);
  if (rc) return rc;
  DeviceGuard g(c->device);
  const size_t set_words = size_t(n_sub) * CABAC_NUM_CONTEXTS;
  if ((rc = ensure(c, kWppState, set_words * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, kWppRate, set_words))) return rc;
  auto *slot_state = static_cast<uint32_t *>(c->d_buf[kWppState]);
  auto *slot_rate = static_cast<uint8_t *>(c->d_buf[kWppRate]);
  uint32_t last = rows.n_level;  // the last non-empty level
  while (last > 0 && rows.level_first[last - 1] == rows.level_first[last]) last--;
  c->timed = false;
  for (uint32_t l = 0; l < last; l++) {
    const uint32_t first = rows.level_first[l], n = rows.level_first[l + 1] - first;
    if (n == 0) continue;
    const bool hands_over = l + 1 < last;
    const cabac::CtxSets sets{n_sub, slot_state, slot_rate, rows.d_sync_from + first, nullptr, slot_state, slot_rate};
    cabac::ParseIn level = in;  // what is per substream starts at the level's first
    level.desc += first;
    level.tile_first += first;
    level.results += first;
    Timed t(c, 35);
    HIP_TRY(c, cabac::launch_plan_parse_sets(c->stream, n, level, sets, rows.d_sync_at + first, first, hands_over ? first : 0xFFFFFFFFu));
  }
  return CABAC_HIP_OK;
}

// ---- the lists of cabac_hip_sparse_encode_batch (cabac_hip_sparse.h) and what that form refuses about them ------------------------
struct SparseSrc {
  const uint32_t *ent_first, *entries;
  uint64_t n_entries;
};

// the first block of [t0, t1) the form refuses, and why (t1: none)
uint32_t first_refused_block(uint32_t t0, uint32_t t1, const cabac_tu_desc *tus, const SparseSrc &sp, const char **why) {
  for (uint32_t t = t0; t < t1; t++) {
    const uint32_t lo = sp.ent_first[t], hi = sp.ent_first[t + 1];
    const char *what = nullptr;
    if (lo > hi) what = "ent_first descends";
    else if (hi > sp.n_entries) what = "ent_first passes n_entries_total";
    else if (tus[t].max_log2_tr_range > 15) what = "max_log2_tr_range above 15 is not carried in the sparse form";
    else if (tus[t].log2_width <= 6 && tus[t].log2_height <= 6) {  // (other sizes: flagged by the binariser, no entry is used)
      const uint32_t n = 1u << (tus[t].log2_width + tus[t].log2_height);
      uint32_t bad = 0;
      for (uint32_t k = lo; k < hi; k++) bad |= uint32_t((sp.entries[k] & 0xFFFFu) >= n);
      if (bad) what = "an entry's pos lies outside the block";
    }
    if (what) {
      *why = what;
      return t;
    }
  }
  return t1;
}

// A large batch is checked by up to eight threads, a slice of the blocks each: the walk is a few nanoseconds per block, which for
// the 1.6 M blocks of the residual tiles is more than the whole upload of their lists takes.
int check_sparse_host(cabac_hip_ctx *c, uint32_t n_tu, const cabac_tu_desc *tus, const SparseSrc &sp) {
  char buf[128];
  if (sp.ent_first[0] != 0u) return fail(c, CABAC_HIP_ERR_INVALID, "block 0: ent_first must start at 0");
  const uint32_t kSlice = 1u << 16;
  const uint32_t n_thread = std::max(1u, std::min({8u, std::thread::hardware_concurrency(), n_tu / kSlice}));
  std::vector<uint32_t> bad(n_thread, n_tu);
  std::vector<const char *> why(n_thread, nullptr);
  auto slice = [&](uint32_t i) {
    const uint32_t t0 = uint32_t(uint64_t(n_tu) * i / n_thread), t1 = uint32_t(uint64_t(n_tu) * (i + 1) / n_thread);
    const uint32_t t = first_refused_block(t0, t1, tus, sp, &why[i]);
    bad[i] = t < t1 ? t : n_tu;
  };
  std::vector<std::thread> workers;
  try {
    for (uint32_t i = 1; i < n_thread; i++) workers.emplace_back(slice, i);
  } catch (...) {  // no thread to be had: the slices that got none are walked here
    for (uint32_t i = (uint32_t)workers.size() + 1; i < n_thread; i++) slice(i);
  }
  slice(0);
  for (std::thread &w : workers) w.join();
  for (uint32_t i = 0; i < n_thread; i++)
    if (bad[i] != n_tu) {  // slices are in block order: the first hit is the lowest block
      snprintf(buf, sizeof buf, "block %u: %s", bad[i], why[i]);
      return fail(c, CABAC_HIP_ERR_INVALID, buf);
    }
  if (sp.ent_first[n_tu] != sp.n_entries) {
    snprintf(buf, sizeof buf, "block %u: ent_first must end at n_entries_total", n_tu);
    return fail(c, CABAC_HIP_ERR_INVALID, buf);
  }
  return CABAC_HIP_OK;
}

// ---- what the host-pointer forms of the parser family (residual, unit, element and plan parse) stage alike: plain copies on the
// ctx stream, no bounce ring, no second stream.  stage() uploads the common inputs and leaves the device views below; the form
// adds its own arrays, launches, fetches its own outputs, and finish() brings back the common ones --------------------------------
struct ParseStage {
  cabac_hip_ctx *c;
  uint32_t n_sub, n_tu;
  int coeff_bytes;
  uint64_t n_coeff_total;
  bool blocks;  // the coefficients go up (int32) or are cleared (int16), and come back
  cabac::ParseIn in{};  // the common operands on the device; the form adds its own members

  size_t tu_word_bytes() const { return size_t(n_tu) * sizeof(uint32_t); }  // one word per block: info words, positions, guards

  // tu_info_in (may be null): the caller's info words go up, so that what the walk does not write comes back as it went in
  int stage(const cabac_substream_desc *desc, const uint8_t *bytes, uint64_t bytes_total, const uint32_t *tile_first,
            const cabac_tu_desc *tus, const void *coeff, const uint32_t *tu_info_in) {
    int rc;
    // kFirstTus: tile_first, padding to 16 bytes, the block descriptors; kBytes: room for the dword that holds the last byte
    const size_t first_bytes = (size_t(n_sub) + 1) * sizeof(uint32_t), first_pad = (first_bytes + 15) / 16 * 16;
    if ((rc = ensure(c, kDesc, n_sub * sizeof(cabac_substream_desc)))) return rc;
    if ((rc = ensure(c, kBytes, bytes_total + 4))) return rc;
    if ((rc = ensure(c, kFirstTus, first_pad + size_t(n_tu) * sizeof(cabac_tu_desc)))) return rc;
    if ((rc = ensure(c, kCoeff, (n_coeff_total + 4) * size_t(coeff_bytes)))) return rc;
    if ((rc = ensure(c, kParseResults, n_sub * sizeof(cabac_substream_result)))) return rc;
    if ((rc = ensure(c, kTuInfo, tu_word_bytes()))) return rc;
    uint8_t *d_first = static_cast<uint8_t *>(c->d_buf[kFirstTus]);
    in = {static_cast<const cabac_substream_desc *>(c->d_buf[kDesc]), static_cast<const uint8_t *>(c->d_buf[kBytes]),
          reinterpret_cast<const uint32_t *>(d_first), reinterpret_cast<const cabac_tu_desc *>(d_first + first_pad), c->d_buf[kCoeff],
          coeff_bytes, static_cast<uint32_t *>(c->d_buf[kTuInfo]), static_cast<cabac_substream_result *>(c->d_buf[kParseResults])};
    HIP_TRY(c, up(c, c->d_buf[kDesc], desc, n_sub * sizeof(cabac_substream_desc)));
    HIP_TRY(c, up(c, c->d_buf[kBytes], bytes, bytes_total));
    HIP_TRY(c, up(c, d_first, tile_first, first_bytes));
    HIP_TRY(c, up(c, d_first + first_pad, tus, size_t(n_tu) * sizeof(cabac_tu_desc)));
    if (tu_info_in) HIP_TRY(c, up(c, in.tu_info, tu_info_in, tu_word_bytes()));
    // int32: what the walk does not write (outside the coded region of 64-wide blocks, the blocks of a stopped substream) keeps
    // the caller's values; int16: output only, zero where nothing is written
    if (blocks && coeff_bytes == 4) HIP_TRY(c, up(c, in.coeff, coeff, n_coeff_total * sizeof(int32_t)));
    if (blocks && n_coeff_total && coeff_bytes == 2) HIP_TRY(c, hipMemsetAsync(in.coeff, 0, n_coeff_total * sizeof(int16_t), c->stream));
    return CABAC_HIP_OK;
  }

  // info words (where the caller wants them), coefficients and results back, the wait, and the flags as the status
  int finish(void *coeff, uint32_t *tu_info, cabac_substream_result *results) {
    if (tu_info) HIP_TRY(c, down(c, tu_info, in.tu_info, tu_word_bytes()));
    if (blocks) HIP_TRY(c, down(c, coeff, in.coeff, n_coeff_total * size_t(coeff_bytes)));
    HIP_TRY(c, down(c, results, in.results, n_sub * sizeof(cabac_substream_result)));
    HIP_TRY(c, wait_stream(c, c->stream));
    int status = CABAC_HIP_OK;
    for (uint32_t s = 0; s < n_sub; s++)
      if (results[s].flags) status = CABAC_HIP_ERR_SUBSTREAM;
    if (status) c->last_error = "substream flag set (see results[].flags)";
    return status;
  }
};

// ---- what the device pipelines of the plan write (the whole write and the write in pieces) set up alike: the sizes and info words of
// the blocks (kSpCnt), the tables of the two walks and their scan (kPwPlan), the expanded descriptors (kSpDesc), the blocks as they
// are coded (kPwTu), their destinations (kSpTuOff); words: two per substream for hand-over records and live out sets (kRowsWords),
// null where the call has no use for them
struct PlanWriteTables {
  uint32_t *cnt, *info;
  uint32_t *sub_n, *sub_cap, *sub_flag, *err;
  uint64_t *rec_base, *byte_base, *totals;
  cabac_substream_desc *desc2;
  cabac_tu_desc *tus2;
  uint64_t *tu_off;
  uint32_t *words;
};
int plan_write_tables(cabac_hip_ctx *c, uint32_t n_sub, uint32_t n_tu, bool with_words, PlanWriteTables *t) {
  int rc;
  const size_t n_blk = n_tu ? n_tu : 1, n_s = n_sub ? n_sub : 1;
  const size_t words = (3 * n_s + 2 + 1) & ~size_t(1);  // sub_n, sub_cap, sub_flag, err (+ pad)
  if (with_words && (rc = ensure(c, kRowsWords, 2 * n_s * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, kSpCnt, 2 * n_blk * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, kResidualScratch, cabac::residual_scratch_bytes(n_tu)))) return rc;
  if ((rc = ensure(c, kPwPlan, words * sizeof(uint32_t) + (2 * n_s + 3) * sizeof(uint64_t)))) return rc;
  if ((rc = ensure(c, kPwTu, n_blk * sizeof(cabac_tu_desc)))) return rc;
  if ((rc = ensure(c, kSpDesc, n_s * sizeof(cabac_substream_desc)))) return rc;
  if ((rc = ensure(c, kSpTuOff, n_blk * sizeof(uint64_t)))) return rc;
  if (!c->ws_fixed && !c->h_totals) HIP_TRY(c, pinned_alloc(c, &c->h_totals, 64, hipHostMallocDefault));
  uint32_t *cnt = static_cast<uint32_t *>(c->d_buf[kSpCnt]);
  uint32_t *sub_n = static_cast<uint32_t *>(c->d_buf[kPwPlan]), *sub_cap = sub_n + n_s, *sub_flag = sub_cap + n_s, *err = sub_flag + n_s;
  uint64_t *rec_base = reinterpret_cast<uint64_t *>(sub_n + words), *byte_base = rec_base + n_s, *totals = byte_base + n_s;
  *t = {cnt, cnt + n_blk, sub_n, sub_cap, sub_flag, err, rec_base, byte_base, totals,
        static_cast<cabac_substream_desc *>(c->d_buf[kSpDesc]), static_cast<cabac_tu_desc *>(c->d_buf[kPwTu]),
        static_cast<uint64_t *>(c->d_buf[kSpTuOff]), with_words ? static_cast<uint32_t *>(c->d_buf[kRowsWords]) : nullptr};
  return CABAC_HIP_OK;
}

// THE ONE WAIT of a pipeline whose sizes decide the buffers of its second half: totals = {records, bytes, refused} as the scan
// left them; refused: the call's message for it.  Then the expanded records (kSpRec) and, where asked, the byte slots (kSpBytes).
int wait_for_totals(cabac_hip_ctx *c, const uint64_t *totals, const char *refused, bool byte_slots) {
  uint64_t *h_tot = static_cast<uint64_t *>(c->h_totals);
  HIP_TRY(c, hipMemcpyAsync(h_tot, totals, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, wait_stream(c, c->stream));
  if (h_tot[2]) return fail(c, CABAC_HIP_ERR_INVALID, refused);
  int rc;
  if ((rc = ensure(c, kSpRec, (h_tot[0] + 64) * sizeof(uint16_t)))) return rc;
  if (byte_slots && (rc = ensure(c, kSpBytes, h_tot[1] + 64))) return rc;
  return CABAC_HIP_OK;
}

// ---- the device calls of the parser family take their operands as a cabac::ParseIn, whose first eight members every walk has.
// The prelude of all but the residual parse (which demands the blocks and has its own): the refusals (args_ok: what the form
// checks beside the common pointers), the empty call, the device, and the launch between its events.  tus / coeff belong to the
// blocks, records / side_bins or plan / values to the runs or plans: either kind may be absent altogether
template <class F>
int parse_device_call(cabac_hip_ctx *c, uint32_t n_sub, const cabac::ParseIn &in, bool args_ok, int kind, const char *what, F &&launch) {
  if (!c || (n_sub && (!in.desc || !in.bytes || !in.tile_first || !in.results)) || !args_ok) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (in.coeff_bytes != 4 && in.coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (n_sub == 0) return CABAC_HIP_OK;
  DeviceGuard g(c->device);
  return timed_launch(c, kind, what, launch);
}
#define PARSE_DEVICE_CALL(c, n_sub, in, args_ok, kind, expr) \
  parse_device_call((c), (n_sub), (in), (args_ok), (kind), #expr, [&] { return (expr); })

// the unit, element and plan walk: one launch, told apart by the walk and its profile kind (25, 26, 27)
int parse_walk_device(cabac_hip_ctx *c, cabac::ParseWalk walk, int kind, uint32_t n_sub, const cabac::ParseIn &in) {
  return PARSE_DEVICE_CALL(c, n_sub, in, true, kind, cabac::launch_parse(c->stream, walk, n_sub, in));
}

}  // namespace

extern "C" {

size_t cabac_hip_encode_bound(uint64_t n_ctx_bins, uint64_t n_ep_bins, uint64_t n_trm_bins) {
  // <= 6 bits per context bin (contexts.cpp:787-789), 1 per bypass bin, <= 7 per terminate bin,
  // finish() <= 2 buffered + 2 flushed bytes, alignment <= 1; rounded up to 16.
  uint64_t bits = 6 * n_ctx_bins + n_ep_bins + 7 * n_trm_bins;
  uint64_t bytes = (bits + 7) / 8 + 8;
  return (size_t)((bytes + 15) / 16 * 16);
}

int cabac_hip_init(int device, cabac_hip_ctx **out) {
  if (!out) return CABAC_HIP_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return CABAC_HIP_ERR_NO_DEVICE;
  if (device < 0 || device >= n) return CABAC_HIP_ERR_INVALID;
  cabac_hip_ctx *c = new (std::nothrow) cabac_hip_ctx;
  if (!c) return CABAC_HIP_ERR_NOMEM;
  c->device = device;
  DeviceGuard g(device);
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&c->ev_start) != hipSuccess || hipEventCreate(&c->ev_stop) != hipSuccess) {
    delete c;
    return CABAC_HIP_ERR_HIP;
  }
  c->own_stream = true;
  if (device_alloc(c, &c->d_select, 256) != hipSuccess) {
    (void)hipGetLastError();
    cabac_hip_destroy(c);
    return CABAC_HIP_ERR_NOMEM;
  }
  *out = c;
  return CABAC_HIP_OK;
}

void cabac_hip_destroy(cabac_hip_ctx *c) {
  if (!c) return;
  DeviceGuard g(c->device);
  (void)wait_stream(c, c->stream);
  while (!c->logs.empty()) (void)cabac_hip_search_log_destroy(c->logs.back());
  for (int i = 0; i < kSlots; i++)
    if (c->d_buf[i]) (void)device_free(c, c->d_buf[i]);
  if (c->h_totals) (void)pinned_free(c, c->h_totals);
  if (c->d_select) (void)device_free(c, c->d_select);
  if (c->d_ws) (void)device_free(c, c->d_ws);
  pipe_destroy(c);
  for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
  if (c->ev_start) (void)hipEventDestroy(c->ev_start);
  if (c->ev_stop) (void)hipEventDestroy(c->ev_stop);
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

const char *cabac_hip_strerror(int status) {
  switch (status) {
  case CABAC_HIP_OK: return "ok";
  case CABAC_HIP_ERR_NO_DEVICE: return "no HIP device (this library has no CPU path)";
  case CABAC_HIP_ERR_INVALID: return "invalid argument";
  case CABAC_HIP_ERR_HIP: return "HIP runtime error";
  case CABAC_HIP_ERR_NOMEM: return "out of memory";
  case CABAC_HIP_ERR_SUBSTREAM: return "a substream reported an error flag";
  default: return "unknown status";
  }
}

const char *cabac_hip_last_error(const cabac_hip_ctx *c) { return c ? c->last_error.c_str() : ""; }

int cabac_hip_set_stream(cabac_hip_ctx *c, void *hip_stream) {
  if (!c) return CABAC_HIP_ERR_INVALID;
  DeviceGuard g(c->device);
  if (c->own_stream && c->stream) {
    (void)wait_stream(c, c->stream);
    (void)hipStreamDestroy(c->stream);
    c->own_stream = false;
    c->stream = nullptr;
  }
  if (hip_stream == CABAC_HIP_STREAM_DEFAULT) {
    c->stream = nullptr;  // the device's default stream (every launch, event and wait below takes a null stream as that)
  } else if (hip_stream) {
    c->stream = (hipStream_t)hip_stream;
  } else {
    HIP_TRY(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->own_stream = true;
  }
  return CABAC_HIP_OK;
}

int cabac_hip_wait_event(cabac_hip_ctx *c, void *hip_event) {
  if (!c || !hip_event) return CABAC_HIP_ERR_INVALID;
  DeviceGuard g(c->device);
  HIP_TRY(c, hipStreamWaitEvent(c->stream, (hipEvent_t)hip_event, 0));
  return CABAC_HIP_OK;
}

int cabac_hip_record_event(cabac_hip_ctx *c, void *hip_event) {
  if (!c || !hip_event) return CABAC_HIP_ERR_INVALID;
  DeviceGuard g(c->device);
  HIP_TRY(c, hipEventRecord((hipEvent_t)hip_event, c->stream));
  return CABAC_HIP_OK;
}

int cabac_hip_synchronize(cabac_hip_ctx *c) {
  if (!c) return CABAC_HIP_ERR_INVALID;
  DeviceGuard g(c->device);
  HIP_TRY(c, wait_stream(c, c->stream));
  return CABAC_HIP_OK;
}

int cabac_hip_set_variant(cabac_hip_ctx *c, int enc, int dec) {
  if (!c) return CABAC_HIP_ERR_INVALID;
  c->enc_variant = enc;
  c->dec_variant = dec;
  return CABAC_HIP_OK;
}

int cabac_hip_encode_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc,
                            const uint16_t *d_records, uint8_t *d_bytes, cabac_substream_result *d_results) {
  if (!c || (n_sub && (!d_desc || !d_records || !d_bytes || !d_results))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  return TIMED_LAUNCH(c, 0, cabac::launch_encode(c->stream, c->enc_variant, n_sub, d_desc, d_records, d_bytes, d_results));
}

int cabac_hip_decode_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc,
                            const uint16_t *d_records, const uint8_t *d_bytes, uint8_t *d_bins,
                            cabac_substream_result *d_results) {
  if (!c || (n_sub && (!d_desc || !d_records || !d_bytes || !d_bins || !d_results)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  return TIMED_LAUNCH(c, 1, cabac::launch_decode(c->stream, c->dec_variant, n_sub, d_desc, d_records, d_bytes, d_bins, d_results, 0, c->d_select));
}

int cabac_hip_estimate_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc,
                              const uint16_t *d_records, uint64_t *d_frac_bits, uint32_t *d_flags) {
  if (!c || (n_sub && (!d_desc || !d_records || !d_frac_bits))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  return TIMED_LAUNCH(c, 4, cabac::launch_estimate(c->stream, n_sub, d_desc, d_records, d_frac_bits, d_flags));
}

int cabac_hip_estimate_from_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc,
                                   const uint16_t *d_records, const uint32_t *d_state, const uint8_t *d_rate,
                                   const uint32_t *d_set, uint64_t *d_frac_bits, uint32_t *d_flags) {
  if (!c || (n_sub && (!d_desc || !d_records || !d_frac_bits || !d_state || !d_rate || !d_set)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  return TIMED_LAUNCH(c, 4, cabac::launch_estimate(c->stream, n_sub, d_desc, d_records, d_frac_bits, d_flags, d_state, d_rate, d_set));
}

int cabac_hip_ctx_init_device(cabac_hip_ctx *c, uint32_t n_sub, const int32_t *d_qp, const uint32_t *d_init_id,
                              uint32_t *d_state, uint8_t *d_rate) {
  if (!c || (n_sub && (!d_qp || !d_init_id || !d_state || !d_rate))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  HIP_TRY(c, cabac::launch_ctx_init(c->stream, n_sub, d_qp, d_init_id, d_state, d_rate));
  return CABAC_HIP_OK;
}

int cabac_hip_profile_enable(cabac_hip_ctx *c, uint32_t capacity) {
  if (!c) return CABAC_HIP_ERR_INVALID;
  DeviceGuard g(c->device);
  (void)wait_stream(c, c->stream);
  for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
  c->prof_ev.clear();
  c->prof_kind.clear();
  c->prof_n = 0;
  for (uint32_t i = 0; i < 2 * capacity; i++) {
    hipEvent_t e;
    HIP_TRY(c, hipEventCreate(&e));
    c->prof_ev.push_back(e);
  }
  c->prof_kind.assign(capacity, 0);
  return CABAC_HIP_OK;
}

int cabac_hip_profile_read(cabac_hip_ctx *c, int32_t *kind, float *ms, uint32_t max_entries) {
  if (!c || !kind || !ms) return CABAC_HIP_ERR_INVALID;
  DeviceGuard g(c->device);
  HIP_TRY(c, wait_stream(c, c->stream));
  uint32_t n = c->prof_n < max_entries ? c->prof_n : max_entries;
  for (uint32_t i = 0; i < n; i++) {
    kind[i] = c->prof_kind[i];
    HIP_TRY(c, hipEventElapsedTime(&ms[i], c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
  }
  c->prof_n = 0;
  return (int)n;
}

int cabac_hip_assemble_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc,
                              const cabac_substream_result *d_results, const uint8_t *d_bytes, uint8_t *d_payload,
                              uint64_t payload_capacity, uint64_t *d_offsets) {
  if (!c || !d_offsets || (n_sub && (!d_desc || !d_results || !d_bytes || !d_payload)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  return TIMED_LAUNCH(c, 6, cabac::launch_assemble(c->stream, n_sub, d_desc, d_results, d_bytes, d_payload, payload_capacity, d_offsets));
}

int cabac_hip_split_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint64_t *d_offsets,
                           const uint8_t *d_payload, uint8_t *d_bytes) {
  if (!c || (n_sub && (!d_desc || !d_offsets || !d_payload || !d_bytes))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  return TIMED_LAUNCH(c, 7, cabac::launch_split(c->stream, n_sub, d_desc, d_offsets, d_payload, d_bytes));
}

int cabac_hip_count_emulations_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc,
                                      const cabac_substream_result *d_results, const uint8_t *d_bytes,
                                      uint32_t *d_counts) {
  if (!c || (n_sub && (!d_desc || !d_results || !d_bytes || !d_counts))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  return TIMED_LAUNCH(c, 8, cabac::launch_count_emulations(c->stream, n_sub, d_desc, d_results, d_bytes, d_counts));
}

int cabac_hip_gather_records_device(cabac_hip_ctx *c, uint32_t n_seg, const uint64_t *d_src_off, const uint64_t *d_dst_off,
                                    const uint32_t *d_len, const uint16_t *d_src, uint16_t *d_dst) {
  if (!c || (n_seg && (!d_src_off || !d_dst_off || !d_len || !d_src || !d_dst))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  HIP_TRY(c, cabac::launch_gather_records(c->stream, n_seg, d_src_off, d_dst_off, d_len, d_src, d_dst));
  c->timed = false;
  return CABAC_HIP_OK;
}

float cabac_hip_last_kernel_ms(cabac_hip_ctx *c) {
  if (!c || !c->timed) return -1.0f;
  DeviceGuard g(c->device);
  if (wait_event(c, c->ev_stop) != hipSuccess) return -1.0f;
  float ms = -1.0f;
  if (hipEventElapsedTime(&ms, c->ev_start, c->ev_stop) != hipSuccess) return -1.0f;
  return ms;
}

// bytes != NULL: every substream's bytes at its byte_offset (the reference's FIFOs); payload != NULL: the substreams back to
// back in descriptor order with payload_offsets[0..n_sub] (what OutputBitstream::addSubstream makes of byte-aligned
// substreams, bit_stream.cpp:139-150).  rec10: `records` are the packed blocks of cabac_hip_rec10.h, CABAC_REC10_BYTES(n_records_total)
// bytes of them, instead of uint16_t[n_records_total]
static int encode_batch_impl(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const void *records,
                             uint64_t n_records_total, uint8_t *bytes, uint64_t bytes_total, uint8_t *payload,
                             uint64_t payload_capacity, uint64_t *payload_offsets, cabac_substream_result *results, bool rec10 = false) {
  if (!c || (n_sub && (!desc || !results))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (payload_offsets) payload_offsets[0] = 0;
  if (n_sub == 0) return CABAC_HIP_OK;
  int rc = check_desc_host(c, n_sub, desc, n_records_total, bytes_total);
  if (rc) return rc;
  DeviceGuard g(c->device);
  if ((rc = pipe_init(c))) return rc;
  const std::vector<Chunk> chunks = plan_chunks(c, n_sub, desc);
  const uint32_t nc = uint32_t(chunks.size());
  // device: kPayload holds chunk k from its byte_lo, kPayloadOffsets n_k + 1 entries per chunk from s0 + k.  pinned: [0] results
  // then offsets, [1] payload.
  const size_t res_bytes = size_t(n_sub) * sizeof(cabac_substream_result);
  const size_t off_count = size_t(n_sub) + nc;
  if ((rc = ensure(c, kDesc, n_sub * sizeof(cabac_substream_desc)))) return rc;
  if ((rc = ensure(c, kRecords, n_records_total * 2))) return rc;
  if (rec10 && (rc = ensure(c, kRec10, CABAC_REC10_BYTES(n_records_total)))) return rc;
  if ((rc = ensure(c, kBytes, bytes_total))) return rc;
  if ((rc = ensure(c, kResults, res_bytes))) return rc;
  if ((rc = ensure(c, kPayload, bytes_total))) return rc;
  if ((rc = ensure(c, kPayloadOffsets, off_count * sizeof(uint64_t)))) return rc;
  if ((rc = ensure_pinned(c, 0, res_bytes + off_count * sizeof(uint64_t)))) return rc;
  auto *d_desc = static_cast<const cabac_substream_desc *>(c->d_buf[kDesc]);
  auto *d_rec = static_cast<uint16_t *>(c->d_buf[kRecords]);
  auto *d_slots = static_cast<uint8_t *>(c->d_buf[kBytes]);
  auto *d_res = static_cast<cabac_substream_result *>(c->d_buf[kResults]);
  auto *d_pay = static_cast<uint8_t *>(c->d_buf[kPayload]);
  auto *d_off = static_cast<uint64_t *>(c->d_buf[kPayloadOffsets]);
  auto *h_res = static_cast<cabac_substream_result *>(c->h_pin[0]);
  auto *h_off = reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(c->h_pin[0]) + res_bytes);

  // what came before on the caller's stream is finished first; everything below runs on the library's own streams
  HIP_TRY(c, wait_stream(c, c->stream));
  if ((rc = h2d(c, c->d_buf[kDesc], desc, n_sub * sizeof(cabac_substream_desc), c->s_in))) return rc;
  for (uint32_t k = 0; k < nc; k++) {
    const Chunk &ch = chunks[k];
    const uint32_t n_k = ch.s1 - ch.s0;
    if ((rc = upload_chunk_records(c, ch, records, rec10, d_rec))) return rc;
    HIP_TRY(c, hipEventRecord(c->ev_in[k], c->s_in));
    hipStream_t ks = c->s_k[k % cabac_hip_ctx::kKernelStreams];
    HIP_TRY(c, hipStreamWaitEvent(ks, c->ev_in[k], 0));
    if (rec10 && (rc = unpack_chunk_records(c, ch, ks, d_rec))) return rc;
    // (timed only through the profile ring: the ctx's single event pair would tie the chunk streams together)
    const bool ring = !c->prof_ev.empty() && c->prof_n < c->prof_kind.size();
    Bracket br = ring ? bracket_for(c, 0) : Bracket{nullptr, nullptr};
    if (ring) HIP_TRY(c, hipEventRecord(br.a, ks));
    HIP_TRY(c, cabac::launch_encode(ks, c->enc_variant, n_k, d_desc + ch.s0, d_rec, d_slots, d_res + ch.s0, n_sub));
    if (ring) HIP_TRY(c, hipEventRecord(br.b, ks));
    c->timed = false;
    // compaction: the coded substreams of the chunk back to back, so that they leave in ONE copy instead of one per
    // substream (the payload is ~0.1 B/bin; the slots are sized for the worst case)
    HIP_TRY(c, cabac::launch_assemble(ks, n_k, d_desc + ch.s0, d_res + ch.s0, d_slots, d_pay + ch.byte_lo,
                                      ch.byte_hi - ch.byte_lo, d_off + ch.s0 + k));
    HIP_TRY(c, hipMemcpyAsync(h_res + ch.s0, d_res + ch.s0, n_k * sizeof(cabac_substream_result), hipMemcpyDeviceToHost, ks));
    HIP_TRY(c, hipMemcpyAsync(h_off + ch.s0 + k, d_off + ch.s0 + k, (size_t(n_k) + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ks));
    HIP_TRY(c, hipEventRecord(c->ev_k[k], ks));
  }
  // the sizes of chunk k are known once its kernel is through: its payload follows while later chunks are still coded
  std::vector<uint64_t> pay_base(nc + 1, 0);
  for (uint32_t k = 0; k < nc; k++) {
    const Chunk &ch = chunks[k];
    HIP_TRY(c, wait_event(c, c->ev_k[k]));
    const uint64_t n_pay = h_off[ch.s1 + k];
    pay_base[k + 1] = pay_base[k] + n_pay;
    if (payload) {  // straight into the caller's payload (DMA if it is pinned, else through the bounce ring)
      if (pay_base[k + 1] > payload_capacity) return fail(c, CABAC_HIP_ERR_INVALID, "payload_capacity too small");
      if ((rc = d2h(c, payload + pay_base[k], d_pay + ch.byte_lo, n_pay, c->s_out))) return rc;
    } else {
      if ((rc = ensure_pinned_keep(c, 1, pay_base[k + 1], pay_base[k]))) return rc;
      if (n_pay)
        HIP_TRY(c, hipMemcpyAsync(static_cast<uint8_t *>(c->h_pin[1]) + pay_base[k], d_pay + ch.byte_lo, n_pay, hipMemcpyDeviceToHost, c->s_out));
    }
    HIP_TRY(c, hipEventRecord(c->ev_out[k], c->s_out));
  }
  if (payload && (rc = d2h_drain(c))) return rc;
  int status = CABAC_HIP_OK;
  for (uint32_t k = 0; k < nc; k++) {
    const Chunk &ch = chunks[k];
    HIP_TRY(c, wait_event(c, c->ev_out[k]));
    const uint8_t *pay = payload ? payload + pay_base[k] : static_cast<const uint8_t *>(c->h_pin[1]) + pay_base[k];
    const uint64_t *off = h_off + ch.s0 + k;
    for (uint32_t s = ch.s0; s < ch.s1; s++) {
      const uint64_t o = off[s - ch.s0], n = off[s - ch.s0 + 1] - o;
      if (n && bytes) std::memcpy(bytes + desc[s].byte_offset, pay + o, n);  // into the caller's slots
      if (payload_offsets) payload_offsets[s + 1] = pay_base[k] + o + n;
      results[s] = h_res[s];
      if (h_res[s].flags) status = CABAC_HIP_ERR_SUBSTREAM;
    }
  }
  if (status) c->last_error = "substream flag set (see results[].flags)";
  return status;
}

int cabac_hip_encode_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                           uint64_t n_records_total, uint8_t *bytes, uint64_t bytes_total,
                           cabac_substream_result *results) {
  return host_call_exit(c, encode_batch_impl(c, n_sub, desc, records, n_records_total, bytes, bytes_total, nullptr, 0, nullptr, results));
}

int cabac_hip_encode_batch_payload(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                   uint64_t n_records_total, uint8_t *payload, uint64_t payload_capacity,
                                   uint64_t *payload_offsets, cabac_substream_result *results) {
  if (!payload || !payload_offsets) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  uint64_t slots_end = 0;  // the device-side slots still follow the descriptors' byte_offset / byte_capacity
  for (uint32_t s = 0; s < n_sub && desc; s++) slots_end = std::max<uint64_t>(slots_end, desc[s].byte_offset + desc[s].byte_capacity);
  return host_call_exit(c, encode_batch_impl(c, n_sub, desc, records, n_records_total, nullptr, slots_end, payload, payload_capacity,
                                             payload_offsets, results));
}

int cabac_hip_estimate_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                             uint64_t n_records_total, uint64_t *frac_bits, uint32_t *flags) {
  if (!c || (n_sub && (!desc || !frac_bits))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (n_sub == 0) return CABAC_HIP_OK;
  for (uint32_t s = 0; s < n_sub; s++)
    if (int bad = check_records_host(c, s, desc[s], n_records_total)) return bad;
  DeviceGuard g(c->device);
  Stage st{c};
  auto *d_desc = st.put(kDesc, n_sub, desc);
  auto *d_rec = st.put(kRecords, n_records_total, records);
  auto *d_bits = st.room<uint64_t>(kFracBits, n_sub);
  auto *d_flags = st.room<uint32_t>(kFlags, n_sub);
  if (st.rc) return st.rc;
  if (int rc = cabac_hip_estimate_device(c, n_sub, d_desc, d_rec, d_bits, d_flags)) return rc;
  std::vector<uint32_t> fl(n_sub);
  HIP_TRY(c, down(c, frac_bits, d_bits, n_sub * sizeof(uint64_t)));
  HIP_TRY(c, down(c, fl.data(), d_flags, n_sub * sizeof(uint32_t)));
  HIP_TRY(c, wait_stream(c, c->stream));
  return flags_status(c, n_sub, fl.data(), flags, "substream flag set (see flags[])");
}

// packed: `bins` receives (n_records_total + 7) / 8 bytes, bit (r & 7) of byte r >> 3 = the bin of record r
// rec10: as for encode_batch_impl
static int decode_batch_impl(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const void *records,
                             uint64_t n_records_total, const uint8_t *bytes, uint64_t bytes_total, uint8_t *bins,
                             cabac_substream_result *results, bool packed, bool rec10 = false) {
  if (!c || (n_sub && (!desc || !results))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (n_sub == 0) return CABAC_HIP_OK;
  int rc = check_desc_host(c, n_sub, desc, n_records_total, bytes_total);
  if (rc) return rc;
  DeviceGuard g(c->device);
  if ((rc = pipe_init(c))) return rc;
  const std::vector<Chunk> chunks = plan_chunks(c, n_sub, desc);
  const uint32_t nc = uint32_t(chunks.size());
  const size_t res_bytes = size_t(n_sub) * sizeof(cabac_substream_result);
  // the kernel reads whole aligned dwords: room for the dword that holds the last byte
  if ((rc = ensure(c, kDesc, n_sub * sizeof(cabac_substream_desc)))) return rc;
  if ((rc = ensure(c, kRecords, n_records_total * 2))) return rc;
  if (rec10 && (rc = ensure(c, kRec10, CABAC_REC10_BYTES(n_records_total)))) return rc;
  if ((rc = ensure(c, kBytes, bytes_total + 4))) return rc;
  if ((rc = ensure(c, kResults, res_bytes))) return rc;
  if ((rc = ensure(c, kBins, n_records_total + 8))) return rc;
  if (packed && bins && (rc = ensure(c, kPackedBins, (n_records_total + 7) / 8 + 8))) return rc;
  if ((rc = ensure_pinned(c, 0, res_bytes))) return rc;
  auto *d_desc = static_cast<const cabac_substream_desc *>(c->d_buf[kDesc]);
  auto *d_rec = static_cast<uint16_t *>(c->d_buf[kRecords]);
  auto *d_slots = static_cast<uint8_t *>(c->d_buf[kBytes]);
  auto *d_res = static_cast<cabac_substream_result *>(c->d_buf[kResults]);
  auto *d_bins = static_cast<uint8_t *>(c->d_buf[kBins]);
  auto *h_res = static_cast<cabac_substream_result *>(c->h_pin[0]);

  HIP_TRY(c, wait_stream(c, c->stream));
  if ((rc = h2d(c, c->d_buf[kDesc], desc, n_sub * sizeof(cabac_substream_desc), c->s_in))) return rc;
  for (uint32_t k = 0; k < nc; k++) {
    const Chunk &ch = chunks[k];
    const uint32_t n_k = ch.s1 - ch.s0;
    if ((rc = upload_chunk_records(c, ch, records, rec10, d_rec))) return rc;
    if (bytes && (rc = h2d(c, d_slots + ch.byte_lo, bytes + ch.byte_lo, ch.byte_hi - ch.byte_lo, c->s_in))) return rc;
    HIP_TRY(c, hipEventRecord(c->ev_in[k], c->s_in));
    hipStream_t ks = c->s_k[k % cabac_hip_ctx::kKernelStreams];
    HIP_TRY(c, hipStreamWaitEvent(ks, c->ev_in[k], 0));
    if (rec10 && (rc = unpack_chunk_records(c, ch, ks, d_rec))) return rc;
    const bool ring = !c->prof_ev.empty() && c->prof_n < c->prof_kind.size();
    Bracket br = ring ? bracket_for(c, 1) : Bracket{nullptr, nullptr};
    if (ring) HIP_TRY(c, hipEventRecord(br.a, ks));
    HIP_TRY(c, cabac::launch_decode(ks, c->dec_variant, n_k, d_desc + ch.s0, d_rec, d_slots, d_bins, d_res + ch.s0, n_sub, c->d_select + 1 + k));
    if (ring) HIP_TRY(c, hipEventRecord(br.b, ks));
    c->timed = false;
    HIP_TRY(c, hipMemcpyAsync(h_res + ch.s0, d_res + ch.s0, n_k * sizeof(cabac_substream_result), hipMemcpyDeviceToHost, ks));
    HIP_TRY(c, hipEventRecord(c->ev_k[k], ks));
    // the decoded bins of the chunk leave while the next chunk is decoded
    HIP_TRY(c, hipStreamWaitEvent(c->s_out, c->ev_k[k], 0));
    if (bins && !packed && (rc = d2h(c, bins + ch.rec_lo, d_bins + ch.rec_lo, ch.rec_hi - ch.rec_lo, c->s_out))) return rc;
  }
  if (bins && packed) {  // all chunks decoded (s_out waits for each of them above): eight bins to a byte, one small copy
    HIP_TRY(c, cabac::launch_pack_bins(c->s_out, n_records_total, d_bins, static_cast<uint8_t *>(c->d_buf[kPackedBins])));
    if ((rc = d2h(c, bins, c->d_buf[kPackedBins], (n_records_total + 7) / 8, c->s_out))) return rc;
  }
  if ((rc = d2h_drain(c))) return rc;
  HIP_TRY(c, wait_stream(c, c->s_out));
  for (uint32_t k = 0; k < nc; k++) HIP_TRY(c, wait_event(c, c->ev_k[k]));
  int status = CABAC_HIP_OK;
  for (uint32_t s = 0; s < n_sub; s++) {
    results[s] = h_res[s];
    if (h_res[s].flags) status = CABAC_HIP_ERR_SUBSTREAM;
  }
  if (status) c->last_error = "substream flag set (see results[].flags)";
  return status;
}

int cabac_hip_decode_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                           uint64_t n_records_total, const uint8_t *bytes, uint64_t bytes_total, uint8_t *bins,
                           cabac_substream_result *results) {
  return host_call_exit(c, decode_batch_impl(c, n_sub, desc, records, n_records_total, bytes, bytes_total, bins, results, false));
}

int cabac_hip_decode_batch_packed(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                  uint64_t n_records_total, const uint8_t *bytes, uint64_t bytes_total, uint8_t *packed_bins,
                                  cabac_substream_result *results) {
  return host_call_exit(c, decode_batch_impl(c, n_sub, desc, records, n_records_total, bytes, bytes_total, packed_bins, results, true));
}

int cabac_hip_binarize_device(cabac_hip_ctx *c, uint32_t n_sub, const uint64_t *d_se_offset, const uint32_t *d_se,
                              const uint64_t *d_rec_offset, uint32_t *d_n_records, uint16_t *d_records) {
  if (!c || (n_sub && (!d_se_offset || !d_se || !d_n_records || (d_records && !d_rec_offset))))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  return TIMED_LAUNCH(c, 2, cabac::launch_binarize(c->stream, n_sub, d_se_offset, d_se, d_rec_offset, d_n_records, d_records));
}

int cabac_hip_residual_device(cabac_hip_ctx *c, uint32_t n_tu, const cabac_tu_desc *d_tu, const int32_t *d_coeff,
                              const uint64_t *d_rec_offset, uint32_t *d_n_records, uint32_t *d_info,
                              uint16_t *d_records) {
  if (!c || (n_tu && (!d_tu || !d_coeff || !d_n_records || (d_records && !d_rec_offset))))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  if (int rc = ensure(c, kResidualScratch, cabac::residual_scratch_bytes(n_tu))) return rc;
  return TIMED_LAUNCH(c, 5, cabac::launch_residual(c->stream, n_tu, d_tu, d_coeff, 4, d_rec_offset, d_n_records, d_info, d_records,
                                                   c->d_buf[kResidualScratch]));
}

int cabac_hip_residual_batch(cabac_hip_ctx *c, uint32_t n_tu, const cabac_tu_desc *tus, const int32_t *coeff,
                             uint64_t n_coeff_total, uint64_t *offsets, uint32_t *info, uint16_t *records,
                             uint64_t records_capacity) {
  if (!c || !offsets || (n_tu && (!tus || !coeff))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  offsets[0] = 0;
  if (n_tu == 0) return CABAC_HIP_OK;
  if (int bad = check_coeff_ranges_host(c, n_tu, tus, n_coeff_total)) return bad;
  DeviceGuard g(c->device);
  int rc;
  // staging: kCounts holds the counts, then the info words
  Stage st{c};
  auto *d_tu = st.put(kDesc, n_tu, tus);
  auto *d_coeff = st.put(kCoeff, n_coeff_total, coeff);
  auto *d_off = st.room<uint64_t>(kRecOffsets, n_tu);
  uint32_t *d_cnt = st.room<uint32_t>(kCounts, 2 * size_t(n_tu));
  if (st.rc) return st.rc;
  uint32_t *d_info = d_cnt + n_tu;
  if ((rc = cabac_hip_residual_device(c, n_tu, d_tu, d_coeff, nullptr, d_cnt, d_info, nullptr))) return rc;
  std::vector<uint32_t> cnt(2 * size_t(n_tu));
  HIP_TRY(c, down(c, cnt.data(), d_cnt, cnt.size() * sizeof(uint32_t)));
  HIP_TRY(c, wait_stream(c, c->stream));
  int status = CABAC_HIP_OK;
  for (uint32_t t = 0; t < n_tu; t++) {
    offsets[t + 1] = offsets[t] + cnt[t];
    if (info) info[t] = cnt[n_tu + t];
    if (cnt[n_tu + t] & (CABAC_TU_INFO_EMPTY | CABAC_TU_INFO_BAD_DESC)) status = CABAC_HIP_ERR_SUBSTREAM;
  }
  if (status) c->last_error = "empty block or bad descriptor (see info[])";
  if (!records) return status;
  if (records_capacity < offsets[n_tu]) return fail(c, CABAC_HIP_ERR_INVALID, "records_capacity too small");
  if (offsets[n_tu] == 0) return status;
  auto *d_rec = st.room<uint16_t>(kOutRecords, offsets[n_tu]);
  st.put(kRecOffsets, n_tu, offsets);
  if (st.rc) return st.rc;
  if ((rc = cabac_hip_residual_device(c, n_tu, d_tu, d_coeff, d_off, d_cnt, d_info, d_rec))) return rc;
  HIP_TRY(c, down(c, records, d_rec, offsets[n_tu] * sizeof(uint16_t)));
  HIP_TRY(c, wait_stream(c, c->stream));
  return status;
}

// this one demands the blocks; the others' prelude is parse_device_call
static int residual_parse_device_impl(cabac_hip_ctx *c, uint32_t n_sub, const cabac::ParseIn &in) {
  if (!c || (n_sub && (!in.desc || !in.bytes || !in.tile_first || !in.tus || !in.coeff || !in.results)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  return TIMED_LAUNCH(c, 9, cabac::launch_parse(c->stream, cabac::ParseWalk::kResidual, n_sub, in));
}

int cabac_hip_residual_parse_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint8_t *d_bytes,
                                    const uint32_t *d_tile_first, const cabac_tu_desc *d_tu, int32_t *d_coeff, uint32_t *d_tu_info,
                                    cabac_substream_result *d_results) {
  return residual_parse_device_impl(c, n_sub, {d_desc, d_bytes, d_tile_first, d_tu, d_coeff, 4, d_tu_info, d_results});
}

int cabac_hip_residual_parse16_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint8_t *d_bytes,
                                      const uint32_t *d_tile_first, const cabac_tu_desc *d_tu, int16_t *d_coeff, uint32_t *d_tu_info,
                                      cabac_substream_result *d_results) {
  return residual_parse_device_impl(c, n_sub, {d_desc, d_bytes, d_tile_first, d_tu, d_coeff, 2, d_tu_info, d_results});
}

static int residual_parse_batch_impl(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *bytes,
                                     uint64_t bytes_total, const uint32_t *tile_first, const cabac_tu_desc *tus, void *coeff, int coeff_bytes,
                                     uint64_t n_coeff_total, uint32_t *tu_info, cabac_substream_result *results) {
  if (!c || (n_sub && (!desc || !bytes || !tile_first || !tus || !coeff || !results))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (n_sub == 0) return CABAC_HIP_OK;
  const uint32_t n_tu = tile_first[n_sub];
  for (uint32_t s = 0; s < n_sub; s++)
    if (int bad = check_substream_host(c, desc[s], tile_first, s, &bytes_total)) return bad;
  if (int bad = check_coeff_ranges_host(c, n_tu, tus, n_coeff_total)) return bad;
  DeviceGuard g(c->device);
  // (this form moves the coefficients whenever there are any, with or without blocks, and never sends the caller's info words up)
  ParseStage st{c, n_sub, n_tu, coeff_bytes, n_coeff_total, n_coeff_total != 0};
  int rc;
  if ((rc = st.stage(desc, bytes, bytes_total, tile_first, tus, coeff, nullptr))) return rc;
  if ((rc = residual_parse_device_impl(c, n_sub, st.in))) return rc;
  return st.finish(coeff, tu_info, results);
}

int cabac_hip_residual_parse_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *bytes,
                                   uint64_t bytes_total, const uint32_t *tile_first, const cabac_tu_desc *tus, int32_t *coeff,
                                   uint64_t n_coeff_total, uint32_t *tu_info, cabac_substream_result *results) {
  return residual_parse_batch_impl(c, n_sub, desc, bytes, bytes_total, tile_first, tus, coeff, 4, n_coeff_total, tu_info, results);
}

int cabac_hip_residual_parse_batch16(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *bytes,
                                     uint64_t bytes_total, const uint32_t *tile_first, const cabac_tu_desc *tus, int16_t *coeff,
                                     uint64_t n_coeff_total, uint32_t *tu_info, cabac_substream_result *results) {
  return residual_parse_batch_impl(c, n_sub, desc, bytes, bytes_total, tile_first, tus, coeff, 2, n_coeff_total, tu_info, results);
}

// ---- spliced substreams read back (declared in cabac_hip_parse_unit.h; the side-walking instantiation of the parser) ----------
int cabac_hip_parse_unit_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint8_t *d_bytes,
                                const uint32_t *d_tile_first, const cabac_tu_desc *d_tu, const uint32_t *d_tu_at,
                                const uint16_t *d_records, void *d_coeff, int coeff_bytes, uint8_t *d_side_bins, uint32_t *d_tu_info,
                                cabac_substream_result *d_results) {
  return parse_walk_device(c, cabac::ParseWalk::kUnit, 25, n_sub,
                           {d_desc, d_bytes, d_tile_first, d_tu, d_coeff, coeff_bytes, d_tu_info, d_results, d_tu_at, nullptr, nullptr,
                            nullptr, d_records, d_side_bins});
}

int cabac_hip_parse_unit_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *bytes,
                               uint64_t bytes_total, const uint32_t *tile_first, const cabac_tu_desc *tus, const uint32_t *tu_at,
                               const uint16_t *records, uint64_t n_records_total, void *coeff, int coeff_bytes, uint64_t n_coeff_total,
                               uint8_t *side_bins, uint32_t *tu_info, cabac_substream_result *results) {
  if (!c || (n_sub && (!desc || !bytes || !tile_first || !results))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (coeff_bytes != 4 && coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (n_sub == 0) return CABAC_HIP_OK;
  const uint32_t n_tu = tile_first[n_sub];
  if (n_tu && (!tus || !coeff)) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (n_records_total && (!records || !side_bins)) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  for (uint32_t s = 0; s < n_sub; s++) {
    if (int bad = check_substream_host(c, desc[s], tile_first, s, &bytes_total)) return bad;
    const uint64_t n_rec = desc[s].n_records;
    if (desc[s].rec_offset > n_records_total || n_rec > n_records_total - desc[s].rec_offset)
      return fail(c, CABAC_HIP_ERR_INVALID, "a side run leaves n_records_total");
    uint32_t at = 0;
    for (uint32_t t = tile_first[s]; tu_at && t < tile_first[s + 1]; t++) {
      if (tu_at[t] < at) return fail(c, CABAC_HIP_ERR_INVALID, "tu_at decreases inside a substream");
      if (tu_at[t] > n_rec) return fail(c, CABAC_HIP_ERR_INVALID, "tu_at exceeds the substream's run length");
      at = tu_at[t];
    }
    for (uint64_t i = 0; i < n_rec; i++) {
      const uint32_t id = records[desc[s].rec_offset + i] & CABAC_REC_ID_MASK;
      if (id >= CABAC_NUM_CONTEXTS && id < CABAC_REC_ALIGN) {
        char buf[160];
        snprintf(buf, sizeof buf, "bad side record: substream %u, record %llu of its run (id 0x%x)", s, (unsigned long long)i, id);
        return fail(c, CABAC_HIP_ERR_INVALID, buf);
      }
    }
  }
  if (int bad = check_coeff_ranges_host(c, n_tu, tus, n_coeff_total)) return bad;
  DeviceGuard g(c->device);
  // the common staging (the caller's info words do not go up); the runs, the positions and the side bins in slots of their own
  ParseStage st{c, n_sub, n_tu, coeff_bytes, n_coeff_total, n_tu != 0};
  int rc;
  if ((rc = st.stage(desc, bytes, bytes_total, tile_first, tus, coeff, nullptr))) return rc;
  Stage own{c};
  st.in.records = own.put(kUnitRecords, n_records_total, records);
  st.in.tu_at = own.opt(kUnitTuAt, n_tu, tu_at);
  st.in.side_bins = own.put(kUnitBins, n_records_total, side_bins);  // what the walk does not write keeps the caller's values
  if (own.rc) return own.rc;
  if ((rc = parse_walk_device(c, cabac::ParseWalk::kUnit, 25, n_sub, st.in))) return rc;
  HIP_TRY(c, down(c, side_bins, st.in.side_bins, n_records_total));
  return st.finish(coeff, tu_info, results);
}

// ---- spliced substreams read back element by element (declared in cabac_hip_parse_elements.h; the element-walking instantiation) ----
int cabac_hip_parse_elements_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint8_t *d_bytes,
                                    const uint32_t *d_tile_first, const cabac_tu_desc *d_tu, const uint32_t *d_tu_at,
                                    const uint32_t *d_tu_guard, const uint32_t *d_plan, void *d_coeff, int coeff_bytes,
                                    uint32_t *d_values, uint32_t *d_tu_info, cabac_substream_result *d_results) {
  return parse_walk_device(c, cabac::ParseWalk::kElement, 26, n_sub,
                           {d_desc, d_bytes, d_tile_first, d_tu, d_coeff, coeff_bytes, d_tu_info, d_results, d_tu_at, d_tu_guard, d_plan, d_values});
}

// ---- a whole transform unit in one walk (declared in cabac_hip_parse_plan.h; the plan-walking instantiation) ----
int cabac_hip_parse_plan_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint8_t *d_bytes,
                                const uint32_t *d_tile_first, const cabac_tu_desc *d_tu, const uint32_t *d_tu_at,
                                const uint32_t *d_tu_guard, const uint32_t *d_plan, void *d_coeff, int coeff_bytes,
                                uint32_t *d_values, uint32_t *d_tu_info, cabac_substream_result *d_results) {
  return parse_walk_device(c, cabac::ParseWalk::kPlan, 27, n_sub,
                           {d_desc, d_bytes, d_tile_first, d_tu, d_coeff, coeff_bytes, d_tu_info, d_results, d_tu_at, d_tu_guard, d_plan, d_values});
}

// what the host-pointer forms of the two refuse about a plan (the plan write and the plan round of the search use it too)
namespace {
// why a plan entry is bad (cabac_hip_parse_elements.h, "A BAD PLAN ENTRY"), or nullptr; i: its index in the substream's plan
const char *bad_plan_entry(uint32_t w0, uint32_t gw, uint64_t i) {
  const uint32_t kind = w0 & 15u, p = w0 >> 4;
  if (kind > CABAC_SE_ALIGN) return "kind above 8";
  if (gw & 0xfc00u) return "reserved guard bits set";
  if ((gw & 0xffu) > i) return "guard reaches in front of the plan";
  switch (kind) {
  case CABAC_SE_CTX_BIN:
    if ((p & 0x1ffu) >= CABAC_NUM_CONTEXTS) return "ctxId above 378";
    break;
  case CABAC_SE_UNARY_MAX:
    if ((p & 0x1ffu) >= CABAC_NUM_CONTEXTS || ((p >> 9) & 0x1ffu) >= CABAC_NUM_CONTEXTS) return "ctxId above 378";
    break;
  case CABAC_SE_EP_BINS:
    if ((p & 63u) > 32u) return "numBins above 32";
    break;
  case CABAC_SE_UNARY_EP:
    if ((p & 63u) > 32u) return "maxSymbol above 32";
    break;
  case CABAC_SE_TRUNC_BIN:
    if (p == 0u) return "maxSymbol 0";
    break;
  case CABAC_SE_REM_ABS: {
    const uint32_t rice = p & 31u, cutoff = (p >> 5) & 31u, ml = (p >> 10) & 63u;
    if (rice > 14u || ml < 15u || ml > 20u || cutoff > 32u - ml) return "REM_ABS parameters outside the defined region";
    break;
  }
  default: break;
  }
  return nullptr;
}

// why an entry of the plan parse is bad, or nullptr; i: its index in the substream's plan, nb: nb(i), the blocks in front of it
const char *bad_computed_entry(uint32_t w0, uint32_t w1, uint64_t i, uint32_t nb) {
  const uint32_t kind = w0 & 15u, p = w0 >> 4;
  if (kind < CABAC_PE_COND) return bad_plan_entry(w0, w1, i);
  if (kind > CABAC_PE_BLOCK_INFO) return "kind above 10";
  if (kind == CABAC_PE_COND) {
    const uint32_t back2 = p & 0xffu, join = (p >> 8) & 3u;
    if (w1 & 0xfc00u) return "reserved test bits set";
    if ((w1 & 0xffu) > i) return "test reaches in front of the plan";
    if (join == 3u) return "join 3";
    if (join != 0u && back2 == 0u) return "a join with back2 0";
    if (join != 0u && back2 > i) return "back2 reaches in front of the plan";
    return nullptr;
  }
  const uint32_t which = p & 15u, shift = (p >> 4) & 31u, width = (p >> 9) & 63u;
  if (w1 & 0xfc00u) return "reserved guard bits set";
  if ((w1 & 0xffu) > i) return "guard reaches in front of the plan";
  if (which >= nb) return "which reaches in front of the substream's blocks";
  if (width == 0u) return "width 0";
  if (shift + width > 32u) return "shift + width above 32";
  return nullptr;
}

// the entry check of the element parse, which has no computed entries and calls word1 the guard
const char *bad_element_entry(uint32_t w0, uint32_t gw, uint64_t i, uint32_t) { return bad_plan_entry(w0, gw, i); }

// which plans a call takes: whether they may hold computed entries, the entry check, what its message calls an entry's second word
struct PlanRules {
  bool computed;
  const char *(*bad_entry)(uint32_t w0, uint32_t w1, uint64_t i, uint32_t nb);
  const char *word1;
};
constexpr PlanRules kElementRules{false, bad_element_entry, "guard"}, kPlanRules{true, bad_computed_entry, "word1"};

// what the host-pointer forms of the element parse, the plan parse and the plan write refuse about descriptors, plan, guards,
// tile_first, tu_at and coefficient ranges; bytes_total: null where the descriptors' byte ranges are not input (the writer); unit:
// what the messages call a descriptor's owner (the plan search describes its candidates this way)
int check_plan_host(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint64_t *bytes_total,
                    const uint32_t *tile_first, const cabac_tu_desc *tus, const uint32_t *tu_at, const uint32_t *tu_guard,
                    const uint32_t *plan, uint64_t n_elements_total, uint64_t n_coeff_total, const PlanRules &rules = kPlanRules,
                    const char *unit = "substream") {
  char buf[200];
  for (uint32_t s = 0; s < n_sub; s++) {
    if (int bad = check_substream_host(c, desc[s], tile_first, s, bytes_total)) return bad;
    const uint64_t n_el = desc[s].n_records;
    if (desc[s].rec_offset > n_elements_total || n_el > n_elements_total - desc[s].rec_offset)
      return fail(c, CABAC_HIP_ERR_INVALID, "a plan leaves n_elements_total");
    uint32_t at = 0;
    for (uint32_t t = tile_first[s]; t < tile_first[s + 1]; t++) {
      if (tu_at) {
        if (tu_at[t] < at) return fail(c, CABAC_HIP_ERR_INVALID, "tu_at decreases inside a substream");
        if (tu_at[t] > n_el) return fail(c, CABAC_HIP_ERR_INVALID, "tu_at exceeds the substream's plan length");
        at = tu_at[t];
      } else {
        at = uint32_t(n_el);
      }
      if (tu_guard && ((tu_guard[t] & 0xfc00u) || (tu_guard[t] & 0xffu) > at)) {
        snprintf(buf, sizeof buf, "bad block guard: %s %u, block %u of its blocks (guard 0x%x at element %u)", unit, s,
                 t - tile_first[s], tu_guard[t], at);
        return fail(c, CABAC_HIP_ERR_INVALID, buf);
      }
    }
    // nb(i): tu_at does not decrease here, so the blocks in front of element i are a prefix of the substream's blocks
    uint32_t t = tile_first[s];
    for (uint64_t i = 0; i < n_el; i++) {
      while (tu_at && t < tile_first[s + 1] && tu_at[t] <= i) t++;
      const uint32_t *e = plan + 2 * (desc[s].rec_offset + i);
      if (const char *why = rules.bad_entry(e[0], e[1], i, t - tile_first[s])) {
        snprintf(buf, sizeof buf, "bad plan entry: %s %u, element %llu of its plan (word0 0x%x, %s 0x%x): %s", unit, s,
                 (unsigned long long)i, e[0], rules.word1, e[1], why);
        return fail(c, CABAC_HIP_ERR_INVALID, buf);
      }
    }
  }
  return check_coeff_ranges_host(c, tile_first[n_sub], tus, n_coeff_total);
}
}  // namespace

// The host-pointer form of the element parse (rules: kElementRules) and of the plan parse.  rows (may be null, the plan parse's
// alone): the levels and the links, all in HOST memory here; the rows parse then takes the plan parse's place
static int parse_plan_batch_impl(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *bytes,
                                 uint64_t bytes_total, const uint32_t *tile_first, const cabac_tu_desc *tus, const uint32_t *tu_at,
                                 const uint32_t *tu_guard, const uint32_t *plan, uint64_t n_elements_total, void *coeff,
                                 int coeff_bytes, uint64_t n_coeff_total, uint32_t *values, uint32_t *tu_info,
                                 cabac_substream_result *results, const PlanRules &rules, const Rows *rows) {
  if (!c || (n_sub && (!desc || !bytes || !tile_first || !results)) || (rows && n_sub && (!rows->d_sync_from || !rows->d_sync_at)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (coeff_bytes != 4 && coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (n_sub == 0) return CABAC_HIP_OK;
  const uint32_t n_tu = tile_first[n_sub];
  if (n_tu && (!tus || !coeff)) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (n_elements_total && (!plan || !values)) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (int bad = check_plan_host(c, n_sub, desc, &bytes_total, tile_first, tus, tu_at, tu_guard, plan, n_elements_total, n_coeff_total, rules))
    return bad;
  if (rows)
    if (int bad = check_rows_host(c, n_sub, *rows)) return bad;
  DeviceGuard g(c->device);
  // the common staging, the caller's info words with it: what the walk does not write keeps the caller's values (int32 blocks,
  // values, info words) or is zero (int16 blocks); the positions, the plan, the block guards and the values in slots of their own
  ParseStage st{c, n_sub, n_tu, coeff_bytes, n_coeff_total, n_tu != 0};
  int rc;
  if ((rc = st.stage(desc, bytes, bytes_total, tile_first, tus, coeff, tu_info))) return rc;
  const size_t value_bytes = size_t(n_elements_total) * sizeof(uint32_t);
  Stage own{c};
  st.in.plan = own.put(kElemPlan, size_t(n_elements_total) * 2, plan);
  st.in.tu_at = own.opt(kUnitTuAt, n_tu, tu_at);
  st.in.tu_guard = own.opt(kElemGuard, n_tu, tu_guard);
  st.in.values = own.put(kElemValues, n_elements_total, values);
  Rows d_rows{};
  if (rows) d_rows = stage_rows(own, n_sub, *rows, false);
  if (own.rc) return own.rc;
  if (rows) {
    rc = parse_rows_device_impl(c, n_sub, st.in, d_rows);
  } else if (rules.computed) {
    rc = parse_walk_device(c, cabac::ParseWalk::kPlan, 27, n_sub, st.in);
  } else {
    rc = parse_walk_device(c, cabac::ParseWalk::kElement, 26, n_sub, st.in);
  }
  if (rc) return rc;
  HIP_TRY(c, down(c, values, st.in.values, value_bytes));
  return st.finish(coeff, tu_info, results);
}

int cabac_hip_parse_elements_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *bytes,
                                   uint64_t bytes_total, const uint32_t *tile_first, const cabac_tu_desc *tus, const uint32_t *tu_at,
                                   const uint32_t *tu_guard, const uint32_t *plan, uint64_t n_elements_total, void *coeff,
                                   int coeff_bytes, uint64_t n_coeff_total, uint32_t *values, uint32_t *tu_info,
                                   cabac_substream_result *results) {
  return parse_plan_batch_impl(c, n_sub, desc, bytes, bytes_total, tile_first, tus, tu_at, tu_guard, plan, n_elements_total, coeff,
                               coeff_bytes, n_coeff_total, values, tu_info, results, kElementRules, nullptr);
}

int cabac_hip_parse_plan_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *bytes,
                               uint64_t bytes_total, const uint32_t *tile_first, const cabac_tu_desc *tus, const uint32_t *tu_at,
                               const uint32_t *tu_guard, const uint32_t *plan, uint64_t n_elements_total, void *coeff,
                               int coeff_bytes, uint64_t n_coeff_total, uint32_t *values, uint32_t *tu_info,
                               cabac_substream_result *results) {
  return parse_plan_batch_impl(c, n_sub, desc, bytes, bytes_total, tile_first, tus, tu_at, tu_guard, plan, n_elements_total, coeff,
                               coeff_bytes, n_coeff_total, values, tu_info, results, kPlanRules, nullptr);
}

// ---- coefficients -> bytes (cabac_splice.hip) -------------------------------------------------------------------
// sets (may be null): the encode launch starts from and writes context sets; rows (may be null): every substream's hand-over pair
// becomes an index into its expanded string and the WPP encode schedule takes the encode launch's place.  Not both.  The plain
// calls pass neither.  d_n_live (the log's emit on a fixed workspace; else null): the device word that says how many of the n_tu
// blocks and n_splice splices count.
static int encode_residual_device_impl(cabac_hip_ctx *c, uint32_t n_sub, const SpliceIn &in, const PayloadOut &out, uint32_t *d_bin_counts,
                                       const cabac::CtxSets *sets = nullptr, const Rows *rows = nullptr, const uint64_t *d_n_live = nullptr,
                                       const SpliceProbes *probes = nullptr) {
  const auto [d_desc, d_records, d_splice_first, d_splices, n_splice, n_tu, d_tu, d_coeff, coeff_bytes] = in;
  const auto [d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info] = out;
  if (!c || !d_payload_offsets || (n_sub && (!d_desc || !d_records || !d_splice_first || !d_payload || !d_results)) ||
      (n_splice && !d_splices) || (n_tu && (!d_tu || !d_coeff)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (probes && n_sub && (!probes->first || (probes->n && (!probes->at || !probes->bits)))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (probes && c->ws_fixed) return fail(c, CABAC_HIP_ERR_INVALID, "the workspace is fixed: the spliced call has no probe form there");
  if (coeff_bytes != 4 && coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (n_splice != n_tu) return fail(c, CABAC_HIP_ERR_INVALID, "every block must be spliced exactly once (n_splice != n_tu)");
  if (rows && n_sub) {
    if (!rows->d_sync_from || !rows->d_sync_at) return fail(c, CABAC_HIP_ERR_INVALID, "null");
    if (int bad = check_levels(c, n_sub, rows->n_level, rows->level_first)) return bad;
  }
  const bool fixed = c->ws_fixed;  // cabac_hip_workspace.h: every ensure below finds its buffer, nothing waits
  if (fixed)
    if (int bad = check_workspace(c, n_sub, n_tu, rows != nullptr)) return bad;
  DeviceGuard g(c->device);
  int rc;
  if ((rows || (fixed && sets)) && (rc = ensure(c, kRowsWords, (fixed ? 2 : 1) * size_t(n_sub ? n_sub : 1) * sizeof(uint32_t)))) return rc;
  const size_t n_pre = size_t(n_splice) + n_sub + 1;
  const size_t plan32 = n_pre + 2 * size_t(n_sub) + size_t(n_tu ? n_tu : 1) + 2;  // pre, sub_n, sub_cap, seen, err (+ pad)
  const size_t plan32_pad = (plan32 + 1) & ~size_t(1);
  if ((rc = ensure(c, kSpCnt, 2 * size_t(n_tu ? n_tu : 1) * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, kResidualScratch, cabac::residual_scratch_bytes(n_tu)))) return rc;
  if ((rc = ensure(c, kSpPlan, plan32_pad * sizeof(uint32_t) + (2 * size_t(n_sub) + 3) * sizeof(uint64_t)))) return rc;
  if ((rc = ensure(c, kSpDesc, size_t(n_sub ? n_sub : 1) * sizeof(cabac_substream_desc)))) return rc;
  if ((rc = ensure(c, kSpTuOff, size_t(n_tu ? n_tu : 1) * sizeof(uint64_t)))) return rc;
  if ((rc = ensure(c, kSpFlag, 64))) return rc;
  if (probes && (rc = ensure(c, kProbeRec, size_t(probes->n ? probes->n : 1) * sizeof(uint32_t)))) return rc;
  if (!fixed && !c->h_totals) HIP_TRY(c, pinned_alloc(c, &c->h_totals, 64, hipHostMallocDefault));
  uint32_t *d_cnt = static_cast<uint32_t *>(c->d_buf[kSpCnt]), *d_info = d_cnt + (n_tu ? n_tu : 1);
  uint32_t *pre = static_cast<uint32_t *>(c->d_buf[kSpPlan]), *sub_n = pre + n_pre, *sub_cap = sub_n + n_sub, *seen = sub_cap + n_sub,
           *err = seen + (n_tu ? n_tu : 1);
  uint64_t *rec_base = reinterpret_cast<uint64_t *>(pre + plan32_pad), *byte_base = rec_base + n_sub, *totals = byte_base + n_sub;
  auto *desc2 = static_cast<cabac_substream_desc *>(c->d_buf[kSpDesc]);
  auto *tu_off = static_cast<uint64_t *>(c->d_buf[kSpTuOff]);
  c->timed = false;
  {  // block sizes (pass 1 of the binariser)
    Timed t(c, 5);
    HIP_TRY(c, cabac::launch_residual(c->stream, n_tu, d_tu, d_coeff, coeff_bytes, nullptr, d_cnt, d_info, nullptr, c->d_buf[kResidualScratch]));
  }
  // fixed: the scan ends in the gate — good or voided, on the device (for a voided call it empties the binariser's block order,
  // which order_ready makes the records pass take as it finds it)
  const cabac::WsGate gate{c->d_ws, CABAC_WS_BAD_SPLICES, nullptr, static_cast<uint32_t *>(c->d_buf[kResidualScratch]),
                           cabac::residual_scratch_bytes(n_tu)};
  {
    Timed t(c, 10);
    HIP_TRY(c, cabac::launch_splice_plan(c->stream, n_sub, n_tu, d_desc, d_splice_first, d_splices, n_splice, d_cnt, pre, sub_n, sub_cap, seen, err,
                                         rec_base, byte_base, totals, d_n_live, fixed ? &gate : nullptr));
  }
  if (!fixed && (rc = wait_for_totals(c, totals, "splice list: not sorted, outside its substream, or a block not spliced exactly once", true)))
    return rc;
  auto *exp_rec = static_cast<uint16_t *>(c->d_buf[kSpRec]);
  auto *slots = static_cast<uint8_t *>(c->d_buf[kSpBytes]);
  {
    Timed t(c, 10);
    if (fixed)
      HIP_TRY(c, cabac::launch_splice_expand_gated(c->stream, c->d_ws, n_sub, d_desc, d_records, d_splice_first, d_splices, pre, sub_n, sub_cap,
                                                   rec_base, byte_base, desc2, tu_off, exp_rec));
    else
      HIP_TRY(c, cabac::launch_splice_expand(c->stream, n_sub, d_desc, d_records, d_splice_first, d_splices, pre, sub_n, sub_cap, rec_base,
                                             byte_base, desc2, tu_off, exp_rec));
  }
  {  // block records (pass 2), straight into the expanded substreams
    Timed t(c, 5);
    HIP_TRY(c, cabac::launch_residual(c->stream, n_tu, d_tu, d_coeff, coeff_bytes, tu_off, d_cnt, d_info, exp_rec, c->d_buf[kResidualScratch],
                                      /*order_ready=*/true));  // the block order of the sizes pass above: same tus[], same scratch
  }
  if (probes && n_sub && probes->n) {  // the pairs as positions in the expanded strings, then the written-bits walk over those strings
    uint32_t *probe_rec = static_cast<uint32_t *>(c->d_buf[kProbeRec]);
    {
      Timed t(c, 47);
      HIP_TRY(c, cabac::launch_splice_probe_index(c->stream, n_sub, probes->n, d_desc, d_splice_first, d_splices, pre, probes->first,
                                                  probes->at, probes->splice, probe_rec));
    }
    Timed t(c, 45);
    HIP_TRY(c, cabac::launch_written_bits(c->stream, n_sub, desc2, exp_rec, cabac::ProbeList{probes->first, probe_rec, 0u}, nullptr, nullptr,
                                          nullptr, probes->bits, nullptr));
  }
  cabac::CtxSets live;  // fixed: a voided call writes no out set
  if (fixed && sets && sets->out_set) {
    uint32_t *out_live = static_cast<uint32_t *>(c->d_buf[kRowsWords]) + (n_sub ? n_sub : 1);
    Timed t(c, 40);
    HIP_TRY(c, cabac::launch_ws_out_sets(c->stream, c->d_ws, n_sub, sets->out_set, out_live));
    live = *sets;
    live.out_set = out_live;
    sets = &live;
  }
  if (rows) {  // the hand-over indices, the context-advance prefix passes per level, then one encode launch from the slots
    uint32_t *sync_rec = static_cast<uint32_t *>(c->d_buf[kRowsWords]);
    {
      Timed t(c, 37);
      if (fixed)
        HIP_TRY(c, cabac::launch_splice_sync_index_gated(c->stream, c->d_ws, n_sub, d_desc, d_splice_first, d_splices, pre, rows->d_sync_at,
                                                         rows->d_sync_splice, sync_rec));
      else
        HIP_TRY(c, cabac::launch_splice_sync_index(c->stream, n_sub, d_desc, d_splice_first, d_splices, pre, rows->d_sync_at,
                                                   rows->d_sync_splice, sync_rec));
    }
    if (n_sub && (rc = wpp_device_impl(c, false, n_sub, desc2, exp_rec, slots, nullptr, d_results, rows->n_level, rows->level_first,
                                       rows->d_sync_from, sync_rec)))
      return rc;
    c->timed = false;
  } else if (sets) {
    Timed t(c, 39);
    HIP_TRY(c, cabac::launch_encode(c->stream, c->enc_variant, n_sub, desc2, exp_rec, slots, d_results, 0, sets));
  } else {
    Timed t(c, 0);
    HIP_TRY(c, cabac::launch_encode(c->stream, c->enc_variant, n_sub, desc2, exp_rec, slots, d_results));
  }
  if (d_bin_counts) {
    Timed t(c, 11);
    HIP_TRY(c, cabac::launch_bin_count(c->stream, n_sub, desc2, exp_rec, d_bin_counts));
  }
  {
    Timed t(c, 6);
    HIP_TRY(c, cabac::launch_assemble(c->stream, n_sub, desc2, d_results, slots, d_payload, payload_capacity, d_payload_offsets,
                                      fixed ? c->d_ws : nullptr, d_results));  // fixed: a voided call's results too
  }
  if (d_tu_info && n_tu) HIP_TRY(c, hipMemcpyAsync(d_tu_info, d_info, size_t(n_tu) * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
  return CABAC_HIP_OK;
}

int cabac_hip_encode_residual_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                     const uint32_t *d_splice_first, const cabac_splice *d_splices, uint32_t n_splice, uint32_t n_tu,
                                     const cabac_tu_desc *d_tu, const int32_t *d_coeff, uint8_t *d_payload, uint64_t payload_capacity,
                                     uint64_t *d_payload_offsets, cabac_substream_result *d_results, uint32_t *d_tu_info,
                                     uint32_t *d_bin_counts) {
  return encode_residual_device_impl(c, n_sub, {d_desc, d_records, d_splice_first, d_splices, n_splice, n_tu, d_tu, d_coeff, 4},
                                     {d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info}, d_bin_counts);
}

int cabac_hip_encode_residual16_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                       const uint32_t *d_splice_first, const cabac_splice *d_splices, uint32_t n_splice, uint32_t n_tu,
                                       const cabac_tu_desc *d_tu, const int16_t *d_coeff, uint8_t *d_payload, uint64_t payload_capacity,
                                       uint64_t *d_payload_offsets, cabac_substream_result *d_results, uint32_t *d_tu_info,
                                       uint32_t *d_bin_counts) {
  return encode_residual_device_impl(c, n_sub, {d_desc, d_records, d_splice_first, d_splices, n_splice, n_tu, d_tu, d_coeff, 2},
                                     {d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info}, d_bin_counts);
}

static int encode_batch_residual_impl(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                      uint64_t n_records_total, const uint32_t *splice_first, const cabac_splice *splices, uint32_t n_tu,
                                      const cabac_tu_desc *tus, const void *coeff, int coeff_bytes, uint64_t n_coeff_total, uint8_t *payload,
                                      uint64_t payload_capacity, uint64_t *payload_offsets, cabac_substream_result *results,
                                      uint32_t *tu_info, uint32_t *bin_counts, const Rows *rows = nullptr,
                                      const SparseSrc *sparse = nullptr, const SpliceProbes *probes = nullptr) {
  if (!c || !payload_offsets || (n_sub && (!desc || !splice_first || !results || !payload)) ||
      (n_tu && (!tus || (!coeff && !sparse) || !splices)) ||
      (rows && n_sub && (!rows->d_sync_from || !rows->d_sync_at)) || (probes && probes->n && !probes->bits))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (c->ws_fixed) return refuse_fixed_batch(c);
  if (coeff_bytes != 4 && coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (probes)  // refused before anything is touched, payload_offsets[0] included
    if (int bad = check_probes_host(c, n_sub, probes->first, probes->at, probes->n)) return bad;
  if (rows && n_sub)
    if (int bad = check_rows_host(c, n_sub, *rows)) return bad;
  if ((!rows && !sparse) || n_sub == 0) payload_offsets[0] = 0;  // (the rows and the sparse form write no output before they have run)
  if (n_sub == 0) return n_tu ? fail(c, CABAC_HIP_ERR_INVALID, "blocks without a substream") : CABAC_HIP_OK;
  for (uint32_t s = 0; s < n_sub; s++)  // (the rows form names the substream)
    if (int bad = check_records_host(c, s, desc[s], n_records_total,
                                     splice_first[s] > splice_first[s + 1] ? "splice_first must not decrease" : nullptr, rows != nullptr))
      return bad;
  const uint32_t n_splice = splice_first[n_sub];
  if (splice_first[0] != 0 || n_splice != n_tu) return fail(c, CABAC_HIP_ERR_INVALID, "every block must be spliced exactly once");
  DeviceGuard g(c->device);
  int rc;
  if ((rc = pipe_init(c))) return rc;
  Stage st{c, true, c->s_in};
  PayloadReturn back{c, n_sub, payload, payload_capacity, payload_offsets, results};
  if ((rc = back.prepare(st, n_tu))) return rc;
  uint32_t *d_counts = bin_counts ? st.room<uint32_t>(kSpOutCnt, size_t(n_sub) * CABAC_BIN_COUNT_WORDS) : nullptr;
  uint32_t *d_flag = st.room<uint32_t>(kSpFlag, 16);  // [0] descriptor range check, [1] empty / bad block
  void *d_sparse_scratch = sparse ? st.bytes(kSparseScratch, cabac::sparse_scratch_bytes(n_tu), nullptr, 0) : nullptr;
  auto *d_sparse_status = sparse ? st.room<cabac_sparse_status>(kSparseStatus, 1) : nullptr;
  if (st.rc) return st.rc;

  // what came before on the caller's stream is finished first; uploads run on the copy stream, the kernels on the ctx's
  HIP_TRY(c, wait_stream(c, c->stream));
  // small things first: the block descriptors are checked on the device while the coefficients are still on the wire
  SpliceIn in{};
  in.d_tu = st.put(kSpInTu, n_tu, tus);
  if (st.rc) return st.rc;
  HIP_TRY(c, hipEventRecord(c->ev_in[0], c->s_in));
  HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_in[0], 0));
  HIP_TRY(c, cabac::launch_tu_range_check(c->stream, n_tu, in.d_tu, n_coeff_total, d_flag));
  HIP_TRY(c, hipMemcpyAsync(back.h_word, d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev_k[0], c->stream));
  in.d_desc = st.put(kSpInDesc, n_sub, desc);
  in.d_splice_first = st.put(kSpInFirst, size_t(n_sub) + 1, splice_first);
  in.d_splices = st.put(kSpInSplice, n_splice, splices);
  in.d_records = st.put(kSpInRec, n_records_total, records, 8);
  in.n_splice = n_splice, in.n_tu = n_tu, in.coeff_bytes = coeff_bytes;
  const uint32_t *d_ent_first = nullptr, *d_entries = nullptr;
  const size_t coeff_room = (n_coeff_total + 4) * size_t(coeff_bytes);
  if (sparse) {  // the lists go up in the coefficients' place
    d_ent_first = st.put(kSparseFirst, size_t(n_tu) + 1, sparse->ent_first);
    d_entries = st.put(kSparseEnt, sparse->n_entries, sparse->entries);
    in.d_coeff = st.bytes(kSpInCoeff, coeff_room, nullptr, 0);
  } else {
    in.d_coeff = st.bytes(kSpInCoeff, coeff_room, coeff, n_coeff_total * size_t(coeff_bytes));
  }
  Rows d_rows{};
  if (rows) d_rows = stage_rows(st, n_sub, *rows, true);
  SpliceProbes d_probes{};
  if (probes)
    d_probes = SpliceProbes{st.put(kProbeFirst, size_t(n_sub) + 1, probes->first), st.put(kProbeAt, probes->n, probes->at),
                            st.opt(kProbeSplice, probes->n, probes->splice), probes->n, st.room<uint32_t>(kProbeOut, probes->n)};
  if (st.rc) return st.rc;
  HIP_TRY(c, hipEventRecord(c->ev_in[1], c->s_in));
  // the lists are checked while they are on the wire: nothing of the pipeline has run and no output is touched when they are refused
  if (sparse && (rc = check_sparse_host(c, n_tu, tus, *sparse))) return rc;
  HIP_TRY(c, wait_event(c, c->ev_k[0]));
  if (*back.h_word) return fail(c, CABAC_HIP_ERR_INVALID, "coefficients out of range");
  HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_in[1], 0));
  if (sparse) {  // every block that lies inside the buffer (checked above) is written whole: zeros, then its entries
    Timed t(c, 41);
    HIP_TRY(c, cabac::launch_sparse_expand(c->stream, n_tu, in.d_tu, d_ent_first, d_entries, sparse->n_entries, const_cast<void *>(in.d_coeff),
                                           coeff_bytes, n_coeff_total, d_sparse_status, d_sparse_scratch));
  }
  if ((rc = encode_residual_device_impl(c, n_sub, in, back.d, d_counts, nullptr, rows ? &d_rows : nullptr, nullptr, probes ? &d_probes : nullptr)))
    return rc;
  HIP_TRY(c, cabac::launch_tu_info_any(c->stream, n_tu, back.d.d_tu_info, d_flag + 1));
  if ((rc = back.fetch(d_flag + 1))) return rc;
  if (tu_info && (rc = d2h(c, tu_info, back.d.d_tu_info, size_t(n_tu) * sizeof(uint32_t), c->s_out))) return rc;
  if (bin_counts && (rc = d2h(c, bin_counts, d_counts, size_t(n_sub) * CABAC_BIN_COUNT_WORDS * sizeof(uint32_t), c->s_out))) return rc;
  if (probes && (rc = d2h(c, probes->bits, d_probes.bits, size_t(probes->first[n_sub]) * sizeof(uint32_t), c->s_out))) return rc;
  return back.finish(*back.h_word ? CABAC_HIP_ERR_SUBSTREAM : CABAC_HIP_OK,
                     "substream flag set, or an empty / badly described block (see results[].flags, tu_info[])");
}

int cabac_hip_encode_batch_residual(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                    uint64_t n_records_total, const uint32_t *splice_first, const cabac_splice *splices, uint32_t n_tu,
                                    const cabac_tu_desc *tus, const int32_t *coeff, uint64_t n_coeff_total, uint8_t *payload,
                                    uint64_t payload_capacity, uint64_t *payload_offsets, cabac_substream_result *results,
                                    uint32_t *tu_info, uint32_t *bin_counts) {
  return host_call_exit(c, encode_batch_residual_impl(c, n_sub, desc, records, n_records_total, splice_first, splices, n_tu, tus, coeff, 4,
                                                      n_coeff_total, payload, payload_capacity, payload_offsets, results, tu_info,
                                                      bin_counts));
}

int cabac_hip_encode_batch_residual16(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                      uint64_t n_records_total, const uint32_t *splice_first, const cabac_splice *splices, uint32_t n_tu,
                                      const cabac_tu_desc *tus, const int16_t *coeff, uint64_t n_coeff_total, uint8_t *payload,
                                      uint64_t payload_capacity, uint64_t *payload_offsets, cabac_substream_result *results,
                                      uint32_t *tu_info, uint32_t *bin_counts) {
  return host_call_exit(c, encode_batch_residual_impl(c, n_sub, desc, records, n_records_total, splice_first, splices, n_tu, tus, coeff, 2,
                                                      n_coeff_total, payload, payload_capacity, payload_offsets, results, tu_info,
                                                      bin_counts));
}

// ---- plan + values -> bytes (cabac_plan_write.hip; declared in cabac_hip_write_plan.h) --------------------------------------
// sets (may be null): the encode launch starts from and writes context sets; rows (may be null): the emit walk notes each
// substream's hand-over record and the WPP encode schedule takes the encode launch's place.  Not both.
// in: the plan write's operands as the kernels take them (cabac::PlanWriteIn; its last two members are filled in here)
static int write_plan_device_impl(cabac_hip_ctx *c, uint32_t n_sub, cabac::PlanWriteIn in, uint32_t n_tu, const void *d_coeff, int coeff_bytes,
                                  const PayloadOut &out, uint32_t *d_values_out, const cabac::CtxSets *sets, const Rows *rows) {
  const auto [d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info] = out;
  const cabac_tu_desc *d_tu = in.tus;
  if (!c || !d_payload_offsets || (n_sub && (!in.desc || !in.tile_first || !d_payload || !d_results)) || (n_tu && (!d_tu || !d_coeff)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (coeff_bytes != 4 && coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (n_sub == 0 && n_tu) return fail(c, CABAC_HIP_ERR_INVALID, "blocks without a substream");
  if (rows && n_sub) {
    if (!rows->d_sync_from || !rows->d_sync_at) return fail(c, CABAC_HIP_ERR_INVALID, "null");
    if (int bad = check_levels(c, n_sub, rows->n_level, rows->level_first)) return bad;
  }
  const bool fixed = c->ws_fixed;  // cabac_hip_workspace.h: every ensure below finds its buffer, nothing waits
  if (fixed)
    if (int bad = check_workspace(c, n_sub, n_tu, rows != nullptr)) return bad;
  DeviceGuard g(c->device);
  int rc;
  PlanWriteTables w;
  if ((rc = plan_write_tables(c, n_sub, n_tu, sets || rows, &w))) return rc;
  // the hand-over records of a rows call; the out sets of the rows that did not stop
  uint32_t *sync_rec = w.words, *out_live = w.words ? w.words + (n_sub ? n_sub : 1) : nullptr;
  in.tu_n_records = w.cnt, in.tu_info = w.info;
  c->timed = false;
  {  // sizes and info words of ALL blocks: they do not depend on the guards, the guards depend on them
    Timed t(c, 5);
    HIP_TRY(c, cabac::launch_residual(c->stream, n_tu, d_tu, d_coeff, coeff_bytes, nullptr, w.cnt, w.info, nullptr, c->d_buf[kResidualScratch]));
  }
  {
    Timed t(c, 28);
    HIP_TRY(c, cabac::launch_plan_resolve(c->stream, n_sub, in, w.sub_n, w.sub_cap, w.sub_flag, w.err));
    // fixed: the scan ends in the gate; a voided call's substreams all become stopped ones (CABAC_RES_OVERFLOW) of length 0,
    // which the emit walk, the out sets, the records pass and the stops below already treat as the contract asks
    const cabac::WsGate gate{c->d_ws, CABAC_WS_RECORDS_32BIT, w.sub_flag, nullptr, 0};
    HIP_TRY(c, cabac::launch_splice_scan(c->stream, n_sub, w.sub_n, w.sub_cap, w.rec_base, w.byte_base, w.err, w.totals, fixed ? &gate : nullptr));
  }
  if (!fixed && (rc = wait_for_totals(c, w.totals, "a substream outgrows 32 bits of records", true))) return rc;
  auto *exp_rec = static_cast<uint16_t *>(c->d_buf[kSpRec]);
  auto *slots = static_cast<uint8_t *>(c->d_buf[kSpBytes]);
  {
    Timed t(c, 28);
    HIP_TRY(c, cabac::launch_plan_emit(c->stream, n_sub, in, w.sub_n, w.sub_cap, w.sub_flag, w.rec_base, w.byte_base, w.desc2, w.tus2, w.tu_off,
                                       exp_rec, d_values_out, d_tu_info, rows ? rows->d_sync_at : nullptr, rows ? sync_rec : nullptr));
    if (sets && sets->out_set) HIP_TRY(c, cabac::launch_plan_out_sets(c->stream, n_sub, w.sub_flag, sets->out_set, out_live));
  }
  {  // block records of the coded blocks, straight into the expanded substreams: in tus2 a skipped block is one the binariser
     // rejects, so it writes nothing whatever its coefficients hold (another list: the block order is made again)
    Timed t(c, 5);
    HIP_TRY(c, cabac::launch_residual(c->stream, n_tu, w.tus2, d_coeff, coeff_bytes, w.tu_off, w.cnt, w.info, exp_rec, c->d_buf[kResidualScratch]));
  }
  if (rows) {  // the context-advance prefix passes per level, then one encode launch from the slots
    if (n_sub && (rc = wpp_device_impl(c, false, n_sub, w.desc2, exp_rec, slots, nullptr, d_results, rows->n_level, rows->level_first,
                                       rows->d_sync_from, sync_rec)))
      return rc;
    c->timed = false;
  } else if (sets) {
    cabac::CtxSets live = *sets;  // a stopped substream has an empty run: it would write a copy of its start set
    if (live.out_set) live.out_set = out_live;
    Timed t(c, 36);
    HIP_TRY(c, cabac::launch_encode(c->stream, c->enc_variant, n_sub, w.desc2, exp_rec, slots, d_results, 0, &live));
  } else {
    Timed t(c, 0);
    HIP_TRY(c, cabac::launch_encode(c->stream, c->enc_variant, n_sub, w.desc2, exp_rec, slots, d_results));
  }
  {
    Timed t(c, 28);
    HIP_TRY(c, cabac::launch_plan_stops(c->stream, n_sub, w.sub_flag, d_results));
  }
  {
    Timed t(c, 6);
    HIP_TRY(c, cabac::launch_assemble(c->stream, n_sub, w.desc2, d_results, slots, d_payload, payload_capacity, d_payload_offsets));
  }
  return CABAC_HIP_OK;
}

int cabac_hip_write_plan_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint32_t *d_plan,
                                const uint32_t *d_values_in, const uint32_t *d_tile_first, uint32_t n_tu, const cabac_tu_desc *d_tu,
                                const uint32_t *d_tu_at, const uint32_t *d_tu_guard, const void *d_coeff, int coeff_bytes,
                                uint8_t *d_payload, uint64_t payload_capacity, uint64_t *d_payload_offsets,
                                cabac_substream_result *d_results, uint32_t *d_values_out, uint32_t *d_tu_info) {
  return write_plan_device_impl(c, n_sub, {d_desc, d_plan, d_values_in, d_tile_first, d_tu, d_tu_at, d_tu_guard}, n_tu, d_coeff, coeff_bytes,
                                {d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info}, d_values_out, nullptr, nullptr);
}

// rows (may be null): the levels and the links, all in HOST memory here
static int write_plan_batch_impl(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint32_t *plan,
                                 const uint32_t *values_in, uint64_t n_elements_total, const uint32_t *tile_first,
                                 const cabac_tu_desc *tus, const uint32_t *tu_at, const uint32_t *tu_guard, const void *coeff,
                                 int coeff_bytes, uint64_t n_coeff_total, uint8_t *payload, uint64_t payload_capacity,
                                 uint64_t *payload_offsets, cabac_substream_result *results, uint32_t *values_out, uint32_t *tu_info,
                                 const Rows *rows = nullptr) {
  if (!c || !payload_offsets || (n_sub && (!desc || !tile_first || !results || !payload)) ||
      (rows && n_sub && (!rows->d_sync_from || !rows->d_sync_at)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (c->ws_fixed) return refuse_fixed_batch(c);
  if (coeff_bytes != 4 && coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (n_sub == 0) {
    payload_offsets[0] = 0;
    return CABAC_HIP_OK;
  }
  const uint32_t n_tu = tile_first[n_sub];
  if (n_tu && (!tus || !coeff)) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (n_elements_total && (!plan || !values_in)) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (int bad = check_plan_host(c, n_sub, desc, nullptr, tile_first, tus, tu_at, tu_guard, plan, n_elements_total, n_coeff_total)) return bad;
  if (rows)
    if (int bad = check_rows_host(c, n_sub, *rows)) return bad;
  DeviceGuard g(c->device);
  int rc;
  if ((rc = pipe_init(c))) return rc;
  Stage st{c, true, c->s_in};
  PayloadReturn back{c, n_sub, payload, payload_capacity, payload_offsets, results};
  if ((rc = back.prepare(st, n_tu))) return rc;

  // what came before on the caller's stream is finished first; uploads run on the copy stream, the kernels on the ctx's
  HIP_TRY(c, wait_stream(c, c->stream));
  cabac::PlanWriteIn in{};
  in.tus = st.put(kSpInTu, n_tu, tus);
  in.desc = st.put(kSpInDesc, n_sub, desc);
  in.tile_first = st.put(kSpInFirst, size_t(n_sub) + 1, tile_first);
  in.tu_at = st.opt(kUnitTuAt, n_tu, tu_at);
  in.tu_guard = st.opt(kElemGuard, n_tu, tu_guard);
  in.plan = st.put(kElemPlan, size_t(n_elements_total) * 2, plan);
  uint32_t *d_values = st.put(kElemValues, n_elements_total, const_cast<uint32_t *>(values_in));
  in.values = d_values;
  const void *d_coeff = st.bytes(kSpInCoeff, (n_coeff_total + 4) * size_t(coeff_bytes), coeff, n_coeff_total * size_t(coeff_bytes));
  Rows d_rows{};
  if (rows) d_rows = stage_rows(st, n_sub, *rows, false);
  if (st.rc) return st.rc;
  HIP_TRY(c, hipEventRecord(c->ev_in[0], c->s_in));
  HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_in[0], 0));
  PayloadOut out = back.d;
  if (!tu_info) out.d_tu_info = nullptr;
  if ((rc = write_plan_device_impl(c, n_sub, in, n_tu, d_coeff, coeff_bytes, out, values_out ? d_values : nullptr, nullptr, rows ? &d_rows : nullptr)))
    return rc;
  if ((rc = back.fetch(nullptr))) return rc;
  // a stopped substream's values and info words are unspecified on the device: the caller's stay what they were
  for (uint32_t s = 0; s < n_sub; s++) {
    if (back.h_res[s].flags & (CABAC_RES_BAD_RECORD | CABAC_RES_BAD_VALUE)) continue;
    if (values_out && desc[s].n_records &&
        (rc = d2h(c, values_out + desc[s].rec_offset, d_values + desc[s].rec_offset, size_t(desc[s].n_records) * sizeof(uint32_t), c->s_out)))
      return rc;
    if (tu_info && tile_first[s + 1] > tile_first[s] &&
        (rc = d2h(c, tu_info + tile_first[s], back.d.d_tu_info + tile_first[s], size_t(tile_first[s + 1] - tile_first[s]) * sizeof(uint32_t),
                  c->s_out)))
      return rc;
  }
  return back.finish(CABAC_HIP_OK, "substream flag set (see results[].flags)");
}

int cabac_hip_write_plan_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint32_t *plan,
                               const uint32_t *values_in, uint64_t n_elements_total, const uint32_t *tile_first,
                               const cabac_tu_desc *tus, const uint32_t *tu_at, const uint32_t *tu_guard, const void *coeff,
                               int coeff_bytes, uint64_t n_coeff_total, uint8_t *payload, uint64_t payload_capacity,
                               uint64_t *payload_offsets, cabac_substream_result *results, uint32_t *values_out, uint32_t *tu_info) {
  return host_call_exit(c, write_plan_batch_impl(c, n_sub, desc, plan, values_in, n_elements_total, tile_first, tus, tu_at, tu_guard,
                                                 coeff, coeff_bytes, n_coeff_total, payload, payload_capacity, payload_offsets, results,
                                                 values_out, tu_info));
}

// ---- pinned host memory for the caller's buffers ------------------------------------------------------------
// ---- the candidates of cabac_hip_estimate_residual_batch and of the search rounds' host-pointer forms: the host checks both run,
// their staging (kEstIn* / kEstOut*, plain copies on the ctx stream) and the way back of what every such call returns
namespace {
struct CandStage {
  cabac_hip_ctx *c;
  uint32_t n_cand;
  const uint32_t *cand_first;
  const cabac_tu_desc *tus;
  const void *coeff;
  int coeff_bytes;
  uint64_t n_coeff_total;
  uint32_t n_sets;
  const uint32_t *set;
  uint32_t n_tu = 0;
  // the device side
  const uint32_t *d_first = nullptr, *d_set = nullptr;
  const cabac_tu_desc *d_tu = nullptr;
  void *d_coeff = nullptr;
  uint32_t *d_state = nullptr, *d_info = nullptr;
  uint8_t *d_rate = nullptr;
  uint64_t *d_bits = nullptr, *d_tu_bits = nullptr;
  std::vector<uint32_t> info;  // the info words as they came back

  int check_lists() const {
    for (uint32_t k = 0; k < n_cand; k++) {
      if (cand_first[k] > cand_first[k + 1]) return fail(c, CABAC_HIP_ERR_INVALID, "cand_first is not non-decreasing");
      if (set[k] >= n_sets) return fail(c, CABAC_HIP_ERR_INVALID, "set out of range");
    }
    return CABAC_HIP_OK;
  }
  // (the lists are through) the blocks the candidates own: there, and inside the coefficients
  int check_blocks() {
    n_tu = cand_first[n_cand];
    if (n_tu && (!tus || !coeff)) return fail(c, CABAC_HIP_ERR_INVALID, "null");
    return check_coeff_ranges_host(c, n_tu - cand_first[0], tus + cand_first[0], n_coeff_total);
  }
  // coeff_up: the bytes of the coefficients that go up
  int stage(Stage &st, const uint32_t *state, const uint8_t *rate, size_t coeff_up) {
    const size_t set_words = size_t(n_sets) * CABAC_NUM_CONTEXTS;
    d_first = st.put(kEstInFirst, size_t(n_cand) + 1, cand_first);
    d_tu = st.put(kEstInTu, n_tu, tus);
    d_coeff = st.bytes(kEstInCoeff, n_coeff_total * size_t(coeff_bytes), coeff, coeff_up);
    d_state = static_cast<uint32_t *>(st.bytes(kEstInState, set_words * sizeof(uint32_t), state, n_cand ? set_words * sizeof(uint32_t) : 0));
    d_rate = static_cast<uint8_t *>(st.bytes(kEstInRate, set_words, rate, n_cand ? set_words : 0));
    d_set = st.put(kEstInSet, n_cand, set);
    d_bits = st.room<uint64_t>(kEstOutBits, size_t(n_cand) + n_tu);
    d_info = st.room<uint32_t>(kEstOutInfo, n_tu);
    if (st.rc) return st.rc;
    d_tu_bits = d_bits + n_cand;
    if (n_tu) {  // blocks no candidate owns keep a defined value
      HIP_TRY(c, hipMemsetAsync(d_tu_bits, 0, size_t(n_tu) * sizeof(uint64_t), c->stream));
      HIP_TRY(c, hipMemsetAsync(d_info, 0, size_t(n_tu) * sizeof(uint32_t), c->stream));
    }
    return CABAC_HIP_OK;
  }
  // queues the way back of the bits and the info words (tu_frac_bits may be null); the caller waits
  int fetch(uint64_t *frac_bits, uint64_t *tu_frac_bits) {
    info = std::vector<uint32_t>(n_tu);
    HIP_TRY(c, down(c, frac_bits, d_bits, size_t(n_cand) * sizeof(uint64_t)));
    if (tu_frac_bits) HIP_TRY(c, down(c, tu_frac_bits, d_tu_bits, size_t(n_tu) * sizeof(uint64_t)));
    HIP_TRY(c, down(c, info.data(), d_info, size_t(n_tu) * sizeof(uint32_t)));
    return CABAC_HIP_OK;
  }
  // (after the wait) the info words to the caller where wanted; judged: an empty or badly described block is the status
  int info_status(uint32_t *tu_info, bool judged) {
    int status = CABAC_HIP_OK;
    for (uint32_t t = 0; t < n_tu; t++) {
      if (tu_info) tu_info[t] = info[t];
      if (judged && (info[t] & (CABAC_TU_INFO_EMPTY | CABAC_TU_INFO_BAD_DESC))) status = CABAC_HIP_ERR_SUBSTREAM;
    }
    if (status) c->last_error = "empty block or bad descriptor (see tu_info[])";
    return status;
  }
};
}  // namespace

// ---- fused residual estimator (cabac_residual_estimate.hip) -------------------------------------------------------
static int estimate_residual_device_impl(cabac_hip_ctx *c, uint32_t n_cand, const uint32_t *d_cand_first, const cabac_tu_desc *d_tu,
                                         const void *d_coeff, int coeff_bytes, const uint32_t *d_state, const uint8_t *d_rate,
                                         const uint32_t *d_set, uint64_t *d_frac_bits, uint64_t *d_tu_frac_bits, uint32_t *d_tu_info) {
  if (!c || (n_cand && (!d_cand_first || !d_tu || !d_coeff || !d_state || !d_rate || !d_set || !d_frac_bits)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (n_cand == 0) return CABAC_HIP_OK;
  DeviceGuard g(c->device);
  if (int rc = ensure(c, kEstScratch, cabac::residual_estimate_scratch_bytes(n_cand))) return rc;
  return TIMED_LAUNCH(c, 12, cabac::launch_residual_estimate(c->stream, n_cand, d_cand_first, d_tu, d_coeff, coeff_bytes, d_state, d_rate, d_set,
                                                             d_frac_bits, d_tu_frac_bits, d_tu_info, c->d_buf[kEstScratch]));
}

int cabac_hip_estimate_residual_device(cabac_hip_ctx *c, uint32_t n_cand, const uint32_t *d_cand_first, const cabac_tu_desc *d_tu,
                                       const int32_t *d_coeff, const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_set,
                                       uint64_t *d_frac_bits, uint64_t *d_tu_frac_bits, uint32_t *d_tu_info) {
  return estimate_residual_device_impl(c, n_cand, d_cand_first, d_tu, d_coeff, 4, d_state, d_rate, d_set, d_frac_bits, d_tu_frac_bits,
                                       d_tu_info);
}

int cabac_hip_estimate_residual16_device(cabac_hip_ctx *c, uint32_t n_cand, const uint32_t *d_cand_first, const cabac_tu_desc *d_tu,
                                         const int16_t *d_coeff, const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_set,
                                         uint64_t *d_frac_bits, uint64_t *d_tu_frac_bits, uint32_t *d_tu_info) {
  return estimate_residual_device_impl(c, n_cand, d_cand_first, d_tu, d_coeff, 2, d_state, d_rate, d_set, d_frac_bits, d_tu_frac_bits,
                                       d_tu_info);
}

int cabac_hip_estimate_residual_batch(cabac_hip_ctx *c, uint32_t n_cand, const uint32_t *cand_first, const cabac_tu_desc *tus,
                                      const void *coeff, int coeff_bytes, uint64_t n_coeff_total, const uint32_t *state,
                                      const uint8_t *rate, uint32_t n_sets, const uint32_t *set, uint64_t *frac_bits,
                                      uint64_t *tu_frac_bits, uint32_t *tu_info) {
  if (!c || (n_cand && (!cand_first || !state || !rate || !set || !frac_bits))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (coeff_bytes != 4 && coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (n_cand == 0) return CABAC_HIP_OK;
  CandStage cs{c, n_cand, cand_first, tus, coeff, coeff_bytes, n_coeff_total, n_sets, set};
  if (int bad = cs.check_lists()) return bad;
  if (int bad = cs.check_blocks()) return bad;
  DeviceGuard g(c->device);
  int rc;
  Stage st{c};
  if ((rc = cs.stage(st, state, rate, n_coeff_total * size_t(coeff_bytes)))) return rc;
  if ((rc = estimate_residual_device_impl(c, n_cand, cs.d_first, cs.d_tu, cs.d_coeff, coeff_bytes, cs.d_state, cs.d_rate, cs.d_set, cs.d_bits,
                                          cs.d_tu_bits, cs.d_info)))
    return rc;
  if ((rc = cs.fetch(frac_bits, tu_frac_bits))) return rc;
  HIP_TRY(c, wait_stream(c, c->stream));
  return cs.info_status(tu_info, true);
}

// ---- emulation prevention (cabac_nal.hip; declared in cabac_hip_nal.h) ---------------------------------------------------
namespace {
int check_offsets_host(cabac_hip_ctx *c, uint32_t n_seg, const uint64_t *offsets) {
  if (offsets[0] != 0) return fail(c, CABAC_HIP_ERR_INVALID, "offsets[0] must be 0");
  for (uint32_t s = 0; s < n_seg; s++)
    if (offsets[s] > offsets[s + 1]) return fail(c, CABAC_HIP_ERR_INVALID, "offsets are not ascending");
  return CABAC_HIP_OK;
}
}  // namespace

size_t cabac_hip_nal_escape_bound(uint64_t n_bytes) { return (size_t)(n_bytes + n_bytes / 2); }

int cabac_hip_nal_escape_device(cabac_hip_ctx *c, uint32_t n_seg, const uint64_t *d_offsets, const uint8_t *d_payload,
                                uint64_t payload_bytes_max, uint8_t *d_nal, uint64_t nal_capacity, uint64_t *d_nal_offsets,
                                cabac_nal_status *d_status) {
  if (!c || !d_status || (n_seg && !d_offsets) || (d_offsets && !d_nal_offsets) || (d_offsets && payload_bytes_max && !d_payload) ||
      (nal_capacity && !d_nal))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  if (!d_offsets) {  // n_seg == 0 and no string at all
    HIP_TRY(c, hipMemsetAsync(d_status, 0, sizeof(cabac_nal_status), c->stream));
    return CABAC_HIP_OK;
  }
  if (int rc = ensure(c, kNalScratch, cabac::nal_scratch_bytes(payload_bytes_max))) return rc;
  return TIMED_LAUNCH(c, 13, cabac::launch_nal_escape(c->stream, n_seg, d_offsets, d_payload, payload_bytes_max, d_nal, nal_capacity, d_nal_offsets,
                                                      d_status, c->d_buf[kNalScratch]));
}

int cabac_hip_nal_unescape_device(cabac_hip_ctx *c, uint32_t n_seg, const uint64_t *d_nal_offsets, const uint8_t *d_nal,
                                  uint64_t nal_bytes_max, uint8_t *d_payload, uint64_t payload_capacity, uint64_t *d_offsets,
                                  uint32_t *d_locations, uint64_t loc_capacity, uint32_t loc_base, cabac_nal_status *d_status) {
  if (!c || !d_status || (n_seg && !d_nal_offsets) || (d_nal_offsets && !d_offsets) || (d_nal_offsets && nal_bytes_max && !d_nal) ||
      (payload_capacity && !d_payload))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  if (!d_nal_offsets) {
    HIP_TRY(c, hipMemsetAsync(d_status, 0, sizeof(cabac_nal_status), c->stream));
    return CABAC_HIP_OK;
  }
  if (int rc = ensure(c, kNalScratch, cabac::nal_scratch_bytes(nal_bytes_max))) return rc;
  return TIMED_LAUNCH(c, 14, cabac::launch_nal_unescape(c->stream, n_seg, d_nal_offsets, d_nal, nal_bytes_max, d_payload, payload_capacity, d_offsets,
                                                        d_locations, loc_capacity, loc_base, d_status, c->d_buf[kNalScratch]));
}

int cabac_hip_nal_escape_batch(cabac_hip_ctx *c, uint32_t n_seg, const uint64_t *offsets, const uint8_t *payload, uint8_t *nal,
                               uint64_t nal_capacity, uint64_t *nal_offsets, cabac_nal_status *status) {
  if (!c || !status || !offsets || !nal_offsets) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (int rc = check_offsets_host(c, n_seg, offsets)) return rc;
  const uint64_t n = offsets[n_seg];
  if ((n && !payload) || (nal_capacity && !nal)) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  int rc;
  const uint64_t cap = std::min<uint64_t>(nal_capacity, cabac_hip_nal_escape_bound(n));   // no result is longer
  const size_t off_bytes = (size_t(n_seg) + 1) * sizeof(uint64_t);
  Stage st{c};
  auto *d_off = st.put(kNalInOff, size_t(n_seg) + 1, offsets);
  auto *d_in = st.put(kNalIn, n, payload);
  auto *d_out = st.room<uint8_t>(kNalOut, cap);
  auto *d_out_off = st.room<uint64_t>(kNalOutOff, size_t(n_seg) + 1);
  auto *d_status = st.room<cabac_nal_status>(kNalStatus, 1);
  if (st.rc) return st.rc;
  if ((rc = cabac_hip_nal_escape_device(c, n_seg, d_off, d_in, n, d_out, cap, d_out_off, d_status))) return rc;
  HIP_TRY(c, down(c, status, d_status, sizeof(cabac_nal_status)));
  HIP_TRY(c, down(c, nal_offsets, d_out_off, off_bytes));
  HIP_TRY(c, wait_stream(c, c->stream));
  HIP_TRY(c, down(c, nal, d_out, std::min<uint64_t>(status->out_bytes, cap)));
  HIP_TRY(c, wait_stream(c, c->stream));
  return CABAC_HIP_OK;
}

int cabac_hip_nal_unescape_batch(cabac_hip_ctx *c, uint32_t n_seg, const uint64_t *nal_offsets, const uint8_t *nal, uint8_t *payload,
                                 uint64_t payload_capacity, uint64_t *offsets, uint32_t *locations, uint64_t loc_capacity,
                                 uint32_t loc_base, cabac_nal_status *status) {
  if (!c || !status || !offsets || !nal_offsets) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (int rc = check_offsets_host(c, n_seg, nal_offsets)) return rc;
  const uint64_t n = nal_offsets[n_seg];
  if ((n && !nal) || (payload_capacity && !payload)) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (locations && n && (n - 1) + loc_base > 0xffffffffull)
    return fail(c, CABAC_HIP_ERR_INVALID, "locations are 32-bit: the NAL string plus loc_base passes 4 GiB");
  DeviceGuard g(c->device);
  int rc;
  const uint64_t cap = std::min<uint64_t>(payload_capacity, n);
  const uint64_t loc_cap = locations ? std::min<uint64_t>(loc_capacity, n / 3) : 0;   // a removal needs two zeros in front of it
  const size_t off_bytes = (size_t(n_seg) + 1) * sizeof(uint64_t);
  Stage st{c};
  auto *d_in_off = st.put(kNalInOff, size_t(n_seg) + 1, nal_offsets);
  auto *d_in = st.put(kNalIn, n, nal);
  auto *d_out = st.room<uint8_t>(kNalOut, cap);
  auto *d_out_off = st.room<uint64_t>(kNalOutOff, size_t(n_seg) + 1);
  auto *d_loc = st.room<uint32_t>(kNalLoc, loc_cap);
  auto *d_status = st.room<cabac_nal_status>(kNalStatus, 1);
  if (st.rc) return st.rc;
  // (loc_capacity as the caller gave it: CABAC_NAL_LOC_OVERFLOW is judged against that; no more than loc_cap can occur)
  if ((rc = cabac_hip_nal_unescape_device(c, n_seg, d_in_off, d_in, n, d_out, cap, d_out_off, locations ? d_loc : nullptr,
                                          locations ? loc_capacity : 0, loc_base, d_status)))
    return rc;
  HIP_TRY(c, down(c, status, d_status, sizeof(cabac_nal_status)));
  HIP_TRY(c, down(c, offsets, d_out_off, off_bytes));
  HIP_TRY(c, wait_stream(c, c->stream));
  HIP_TRY(c, down(c, payload, d_out, std::min<uint64_t>(status->out_bytes, cap)));
  HIP_TRY(c, down(c, locations, d_loc, std::min<uint64_t>(status->n_changed, loc_cap) * sizeof(uint32_t)));
  HIP_TRY(c, wait_stream(c, c->stream));
  return CABAC_HIP_OK;
}

int cabac_hip_encode_batch_nal(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                               uint64_t n_records_total, uint8_t *nal, uint64_t nal_capacity, uint64_t *nal_offsets,
                               cabac_substream_result *results, cabac_nal_status *status) {
  if (!c || !status || !nal_offsets || (nal_capacity && !nal) || (n_sub && (!desc || !results)) || (n_records_total && !records))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  *status = cabac_nal_status{0, 0, 0};
  nal_offsets[0] = 0;
  if (n_sub == 0) return CABAC_HIP_OK;
  uint64_t slots_end = 0;  // the device-side slots follow the descriptors' byte_offset / byte_capacity, as in cabac_hip_encode_batch_payload
  for (uint32_t s = 0; s < n_sub; s++) slots_end = std::max<uint64_t>(slots_end, desc[s].byte_offset + desc[s].byte_capacity);
  int rc = check_desc_host(c, n_sub, desc, n_records_total, slots_end);
  if (rc) return rc;
  DeviceGuard g(c->device);
  // device: the slots of cabac_hip_encode_batch, then the escape's own
  const size_t off_bytes = (size_t(n_sub) + 1) * sizeof(uint64_t), res_bytes = size_t(n_sub) * sizeof(cabac_substream_result);
  const uint64_t cap = std::min<uint64_t>(nal_capacity, cabac_hip_nal_escape_bound(slots_end));
  Stage st{c};
  auto *d_desc = st.put(kDesc, n_sub, desc);
  auto *d_rec = st.put(kRecords, n_records_total, records);
  auto *d_slots = st.room<uint8_t>(kBytes, slots_end);
  auto *d_res = st.room<cabac_substream_result>(kResults, n_sub);
  auto *d_pay = st.room<uint8_t>(kPayload, slots_end);
  auto *d_off = st.room<uint64_t>(kPayloadOffsets, size_t(n_sub) + 1);
  auto *d_nal = st.room<uint8_t>(kNalOut, cap);
  auto *d_nal_off = st.room<uint64_t>(kNalOutOff, size_t(n_sub) + 1);
  auto *d_status = st.room<cabac_nal_status>(kNalStatus, 1);
  if (st.rc) return st.rc;
  if ((rc = cabac_hip_encode_device(c, n_sub, d_desc, d_rec, d_slots, d_res))) return rc;
  if ((rc = cabac_hip_assemble_device(c, n_sub, d_desc, d_res, d_slots, d_pay, slots_end, d_off))) return rc;
  if ((rc = cabac_hip_nal_escape_device(c, n_sub, d_off, d_pay, slots_end, d_nal, cap, d_nal_off, d_status))) return rc;
  HIP_TRY(c, down(c, status, d_status, sizeof(cabac_nal_status)));
  HIP_TRY(c, down(c, nal_offsets, d_nal_off, off_bytes));
  HIP_TRY(c, down(c, results, d_res, res_bytes));
  HIP_TRY(c, wait_stream(c, c->stream));
  if (status->out_bytes > nal_capacity) return fail(c, CABAC_HIP_ERR_INVALID, "nal_capacity too small (status->out_bytes is the size needed)");
  HIP_TRY(c, down(c, nal, d_nal, status->out_bytes));
  HIP_TRY(c, wait_stream(c, c->stream));
  return flags_status(c, n_sub, results, results, "substream flag set (see results[].flags)");
}

// ---- search rounds (cabac_search.hip, cabac_residual_estimate.hip; declared in cabac_hip_search.h) -----------------------------
namespace {
// the side records of the host-pointer form of cabac_hip_search_unit.h (null: the round of cabac_hip_search.h)
struct HostSide {
  const uint16_t *records;
  uint64_t n_records_total;
  const uint64_t *rec_first;
  const uint32_t *tu_at;
};

// the plans of the host-pointer form of cabac_hip_search_plan.h (null: one of the other two rounds)
struct HostPlan {
  const uint32_t *plan, *values_in;
  uint64_t n_entries_total;
  const uint64_t *ent_first;
  const uint32_t *tu_at, *tu_guard;
  uint32_t *flags, *values_out;
};

// the most bins a value in its domain makes of an entry that is not bad (cabac_hip_search_plan.h, "THE MOST BINS")
uint32_t plan_entry_max_bins(uint32_t w0) {
  const uint32_t kind = w0 & 15u, p = w0 >> 4;
  switch (kind) {
  case CABAC_SE_CTX_BIN:
  case CABAC_SE_TRM:
  case CABAC_SE_ALIGN: return 1;
  case CABAC_SE_EP_BINS:
  case CABAC_SE_UNARY_EP: return p & 63u;
  case CABAC_SE_UNARY_MAX: return (p >> 18) & 0xffu;
  case CABAC_SE_TRUNC_BIN: {
    uint32_t l = 0;
    while ((p >> l) > 1u) l++;
    return l + 1;
  }
  case CABAC_SE_EXP_GOLOMB: return 63u - (p & 31u);
  case CABAC_SE_REM_ABS: {
    const uint32_t rice = p & 31u, cutoff = (p >> 5) & 31u, longest = 32u - cutoff - ((p >> 10) & 63u);
    return std::max(32u, cutoff + rice + (longest ? 2u * longest - 1u : 0u));
  }
  default: return 0;  // computed entries
  }
}

// what cabac_hip_search_plan.h refuses on top of the other rounds; *record_bound: the most records the plans can resolve to
int check_search_plan_host(cabac_hip_ctx *c, uint32_t n_cand, const uint32_t *cand_first, const cabac_tu_desc *tus, const HostPlan &hp,
                           uint64_t n_coeff_total, uint64_t *record_bound) {
  if (!hp.ent_first || (hp.n_entries_total && (!hp.plan || !hp.values_in))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  for (uint32_t k = 0; k < n_cand; k++)
    if (hp.ent_first[k] > hp.ent_first[k + 1]) return fail(c, CABAC_HIP_ERR_INVALID, "ent_first is not non-decreasing");
  if (hp.ent_first[n_cand] > hp.n_entries_total) return fail(c, CABAC_HIP_ERR_INVALID, "ent_first ends past n_entries_total");
  // the plans as the plan write's check sees them: one descriptor per candidate
  std::vector<cabac_substream_desc> desc(n_cand);
  for (uint32_t k = 0; k < n_cand; k++) {
    const uint64_t n_ent = hp.ent_first[k + 1] - hp.ent_first[k];
    if (n_ent > 0xffffffffull) return fail(c, CABAC_HIP_ERR_INVALID, "ent_first: a plan longer than 2^32 - 1 entries");
    uint32_t at = 0;
    for (uint32_t t = cand_first[k]; hp.tu_at && t < cand_first[k + 1]; t++) {
      if (hp.tu_at[t] < at) return fail(c, CABAC_HIP_ERR_INVALID, "tu_at decreases inside a candidate");
      if (hp.tu_at[t] > n_ent) return fail(c, CABAC_HIP_ERR_INVALID, "tu_at exceeds the candidate's plan length");
      at = hp.tu_at[t];
    }
    desc[k] = cabac_substream_desc{};
    desc[k].rec_offset = hp.ent_first[k];
    desc[k].n_records = uint32_t(n_ent);
  }
  if (int bad = check_plan_host(c, n_cand, desc.data(), nullptr, cand_first, tus, hp.tu_at, hp.tu_guard, hp.plan, hp.n_entries_total,
                                n_coeff_total, kPlanRules, "candidate"))
    return bad;
  uint64_t bound = 0;
  for (uint64_t i = hp.ent_first[0]; i < hp.ent_first[n_cand]; i++) bound += plan_entry_max_bins(hp.plan[2 * i]);
  *record_bound = bound;
  return CABAC_HIP_OK;
}

// what the search rounds' host-pointer forms stage beside the candidates: the groups, their out sets and the distortions (either may
// be left out), and where the picks and their costs land
struct SearchStage {
  const uint32_t *group_first, *out_set;
  const uint64_t *dist;
  uint32_t *pick;
  uint64_t *cost;
};

// the plan inputs staged behind what search_round_batch_impl has staged, the resolved form in the library's own buffers (the
// record buffer sized from the bound), and the round
int search_plan_stage_and_run(const CandStage &cs, const SearchStage &ss, uint32_t n_group, const HostPlan &hp, uint64_t record_bound,
                              uint64_t lambda_q16) {
  cabac_hip_ctx *c = cs.c;
  const uint32_t n_cand = cs.n_cand, n_tu = cs.n_tu;
  Stage st{c};
  auto *d_plan = st.put(kElemPlan, size_t(hp.n_entries_total) * 2, hp.plan);
  auto *d_values = st.put(kElemValues, hp.n_entries_total, const_cast<uint32_t *>(hp.values_in));
  auto *d_ent = st.put(kPsEnt, size_t(n_cand) + 1, hp.ent_first);
  auto *d_at = st.opt(kUnitTuAt, n_tu, hp.tu_at);
  auto *d_guard = st.opt(kElemGuard, n_tu, hp.tu_guard);
  auto *d_flags = st.room<uint32_t>(kPsFlags, n_cand ? n_cand : 1);
  auto *d_rec = st.room<uint16_t>(kSearchInRecords, record_bound);
  auto *d_rec_first = st.room<uint64_t>(kSearchInRecFirst, size_t(n_cand) + 1);
  auto *d_at_out = st.room<uint32_t>(kSearchInTuAt, n_tu);
  auto *d_tu_out = st.room<cabac_tu_desc>(kPwTu, n_tu ? n_tu : 1);
  if (st.rc) return st.rc;
  return cabac_hip_search_plan_round_device(c, n_group, ss.group_first, n_cand, cs.d_first, n_tu, cs.d_tu, cs.d_coeff, cs.coeff_bytes, cs.d_state,
                                            cs.d_rate, cs.d_set, d_ent, d_plan, d_values, d_at, d_guard, ss.out_set, ss.dist, lambda_q16,
                                            cs.d_bits, ss.pick, ss.cost, cs.d_tu_bits, cs.d_info, d_flags, d_rec_first, d_rec, record_bound,
                                            d_at_out, d_tu_out, hp.values_out ? d_values : nullptr, nullptr);
}

// the flags and the filled values back; a candidate with a flag is the status
int search_plan_fetch(cabac_hip_ctx *c, uint32_t n_cand, const HostPlan &hp) {
  std::vector<uint32_t> fl(n_cand);
  HIP_TRY(c, down(c, fl.data(), c->d_buf[kPsFlags], size_t(n_cand) * sizeof(uint32_t)));
  if (hp.values_out) HIP_TRY(c, down(c, hp.values_out, c->d_buf[kElemValues], size_t(hp.n_entries_total) * sizeof(uint32_t)));
  HIP_TRY(c, wait_stream(c, c->stream));
  return flags_status(c, n_cand, fl.data(), hp.flags, "a candidate has a flag set (see flags[])");
}

int estimate_residual_ctx_device_impl(cabac_hip_ctx *c, uint32_t n_cand, const uint32_t *d_cand_first, const cabac_tu_desc *d_tu,
                                      const void *d_coeff, int coeff_bytes, const uint32_t *d_state, const uint8_t *d_rate,
                                      const uint32_t *d_set, uint64_t *d_frac_bits, uint64_t *d_tu_frac_bits, uint32_t *d_tu_info,
                                      const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate) {
  if (!c || (n_cand && (!d_cand_first || !d_tu || !d_coeff || !d_state || !d_rate || !d_set || !d_frac_bits || !d_out_set ||
                        !d_out_state || !d_out_rate)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (n_cand == 0) return CABAC_HIP_OK;
  DeviceGuard g(c->device);
  if (int rc = ensure(c, kEstScratch, cabac::residual_estimate_scratch_bytes(n_cand))) return rc;
  return TIMED_LAUNCH(c, 15, cabac::launch_residual_estimate_export(c->stream, n_cand, nullptr, n_cand, d_cand_first, d_tu, d_coeff, coeff_bytes, d_state,
                                                                    d_rate, d_set, d_out_set, d_out_state, d_out_rate, d_frac_bits, d_tu_frac_bits,
                                                                    d_tu_info, c->d_buf[kEstScratch]));
}
}  // namespace

int cabac_hip_estimate_residual_ctx_device(cabac_hip_ctx *c, uint32_t n_cand, const uint32_t *d_cand_first, const cabac_tu_desc *d_tu,
                                           const int32_t *d_coeff, const uint32_t *d_state, const uint8_t *d_rate,
                                           const uint32_t *d_set, uint64_t *d_frac_bits, uint64_t *d_tu_frac_bits, uint32_t *d_tu_info,
                                           const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate) {
  return estimate_residual_ctx_device_impl(c, n_cand, d_cand_first, d_tu, d_coeff, 4, d_state, d_rate, d_set, d_frac_bits,
                                           d_tu_frac_bits, d_tu_info, d_out_set, d_out_state, d_out_rate);
}

int cabac_hip_estimate_residual_ctx16_device(cabac_hip_ctx *c, uint32_t n_cand, const uint32_t *d_cand_first, const cabac_tu_desc *d_tu,
                                             const int16_t *d_coeff, const uint32_t *d_state, const uint8_t *d_rate,
                                             const uint32_t *d_set, uint64_t *d_frac_bits, uint64_t *d_tu_frac_bits,
                                             uint32_t *d_tu_info, const uint32_t *d_out_set, uint32_t *d_out_state,
                                             uint8_t *d_out_rate) {
  return estimate_residual_ctx_device_impl(c, n_cand, d_cand_first, d_tu, d_coeff, 2, d_state, d_rate, d_set, d_frac_bits,
                                           d_tu_frac_bits, d_tu_info, d_out_set, d_out_state, d_out_rate);
}

int cabac_hip_search_select_device(cabac_hip_ctx *c, uint32_t n_group, const uint32_t *d_group_first, const uint64_t *d_frac_bits,
                                   const uint64_t *d_dist, uint64_t lambda_q16, uint32_t *d_pick, uint64_t *d_cost) {
  if (!c || (n_group && (!d_group_first || !d_frac_bits || !d_pick || !d_cost))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (n_group == 0) return CABAC_HIP_OK;
  DeviceGuard g(c->device);
  return TIMED_LAUNCH(c, 16, cabac::launch_search_select(c->stream, n_group, 0xffffffffu, d_group_first, d_frac_bits, d_dist, lambda_q16, d_pick, d_cost));
}

int cabac_hip_search_round_device(cabac_hip_ctx *c, uint32_t n_group, const uint32_t *d_group_first, uint32_t n_cand,
                                  const uint32_t *d_cand_first, const cabac_tu_desc *d_tu, const void *d_coeff, int coeff_bytes,
                                  uint32_t *d_state, uint8_t *d_rate, const uint32_t *d_set, const uint32_t *d_group_out_set,
                                  const uint64_t *d_dist, uint64_t lambda_q16, uint64_t *d_frac_bits, uint32_t *d_pick,
                                  uint64_t *d_cost, uint64_t *d_tu_frac_bits, uint32_t *d_tu_info) {
  if (!c || (n_cand && (!d_cand_first || !d_tu || !d_coeff || !d_state || !d_rate || !d_set || !d_frac_bits)) ||
      (n_group && (!d_group_first || !d_pick || !d_cost)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (coeff_bytes != 4 && coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (n_cand == 0 && n_group == 0) return CABAC_HIP_OK;
  DeviceGuard g(c->device);
  if (int rc = ensure(c, kEstScratch, cabac::residual_estimate_scratch_bytes(std::max(n_cand, n_group)))) return rc;
  c->timed = false;  // three brackets: read them with cabac_hip_profile_read
  // estimate: every candidate from its start set; the sets are not modified
  Bracket br = bracket_for(c, 17);
  HIP_TRY(c, hipEventRecord(br.a, c->stream));
  HIP_TRY(c, cabac::launch_residual_estimate(c->stream, n_cand, d_cand_first, d_tu, d_coeff, coeff_bytes, d_state, d_rate, d_set,
                                             d_frac_bits, d_tu_frac_bits, d_tu_info, c->d_buf[kEstScratch]));
  HIP_TRY(c, hipEventRecord(br.b, c->stream));
  if (n_group == 0) return CABAC_HIP_OK;
  // select
  br = bracket_for(c, 16);
  HIP_TRY(c, hipEventRecord(br.a, c->stream));
  HIP_TRY(c, cabac::launch_search_select(c->stream, n_group, n_cand, d_group_first, d_frac_bits, d_dist, lambda_q16, d_pick, d_cost));
  HIP_TRY(c, hipEventRecord(br.b, c->stream));
  // commit: the picked candidates walked once more by the exporting kernel (d_pick is its index list, CABAC_SEARCH_NONE is
  // skipped); the candidate order of the estimate pass is no longer needed, so the scratch is reused
  br = bracket_for(c, 18);
  HIP_TRY(c, hipEventRecord(br.a, c->stream));
  if (d_group_out_set && n_cand)
    HIP_TRY(c, cabac::launch_residual_estimate_export(c->stream, n_group, d_pick, n_cand, d_cand_first, d_tu, d_coeff, coeff_bytes,
                                                      d_state, d_rate, d_set, d_group_out_set, d_state, d_rate, nullptr, nullptr, nullptr,
                                                      c->d_buf[kEstScratch]));
  HIP_TRY(c, hipEventRecord(br.b, c->stream));
  return CABAC_HIP_OK;
}

static int search_round_batch_impl(cabac_hip_ctx *c, uint32_t n_group, const uint32_t *group_first, uint32_t n_cand,
                                   const uint32_t *cand_first, const cabac_tu_desc *tus, const void *coeff, int coeff_bytes,
                                   uint64_t n_coeff_total, uint32_t *state, uint8_t *rate, uint32_t n_sets, const uint32_t *set,
                                   const uint32_t *group_out_set, const uint64_t *dist, uint64_t lambda_q16, uint64_t *frac_bits,
                                   uint32_t *pick, uint64_t *cost, uint64_t *tu_frac_bits, uint32_t *tu_info, const HostSide *side,
                                   const HostPlan *hp = nullptr) {
  if (!c || !group_first || !cand_first || (n_cand && (!state || !rate || !set || !frac_bits)) || (n_group && (!pick || !cost)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (coeff_bytes != 4 && coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  CandStage cs{c, n_cand, cand_first, tus, coeff, coeff_bytes, n_coeff_total, n_sets, set};
  if (int bad = cs.check_lists()) return bad;
  for (uint32_t g = 0; g < n_group; g++)
    if (group_first[g] > group_first[g + 1]) return fail(c, CABAC_HIP_ERR_INVALID, "group_first is not non-decreasing");
  if (group_first[n_group] != n_cand) return fail(c, CABAC_HIP_ERR_INVALID, "group_first[n_group] must be n_cand");
  if (int bad = cs.check_blocks()) return bad;
  const uint32_t n_tu = cs.n_tu;
  if (group_out_set) {  // the in-place rule of cabac_hip_search.h
    std::vector<uint32_t> owner(n_sets, CABAC_SEARCH_NONE);  // set -> the group that writes it
    for (uint32_t g = 0; g < n_group; g++) {
      const uint32_t o = group_out_set[g];
      if (o == CABAC_SEARCH_NO_SET) continue;
      if (o >= n_sets) return fail(c, CABAC_HIP_ERR_INVALID, "out set out of range");
      if (owner[o] != CABAC_SEARCH_NONE) return fail(c, CABAC_HIP_ERR_INVALID, "two groups name the same out set");
      owner[o] = g;
    }
    uint32_t g = 0;
    for (uint32_t k = 0; k < n_cand; k++) {
      while (g < n_group && group_first[g + 1] <= k) g++;
      const uint32_t mine = (g < n_group && group_first[g] <= k) ? g : CABAC_SEARCH_NONE;  // candidates before group 0 are in no group
      const uint32_t w = owner[set[k]];
      if (w != CABAC_SEARCH_NONE && w != mine) {
        char buf[160];
        snprintf(buf, sizeof buf, "in-place rule: set %u is the out set of group %u and the start set of candidate %u of another group",
                 set[k], w, k);
        return fail(c, CABAC_HIP_ERR_INVALID, buf);
      }
    }
  }
  if (side) {  // what cabac_hip_search_unit.h refuses on top
    if (!side->rec_first || (side->n_records_total && !side->records)) return fail(c, CABAC_HIP_ERR_INVALID, "null");
    for (uint32_t k = 0; k < n_cand; k++)
      if (side->rec_first[k] > side->rec_first[k + 1]) return fail(c, CABAC_HIP_ERR_INVALID, "rec_first is not non-decreasing");
    if (side->rec_first[n_cand] > side->n_records_total) return fail(c, CABAC_HIP_ERR_INVALID, "rec_first ends past n_records_total");
    for (uint32_t k = 0; k < n_cand; k++) {
      const uint64_t n_rec = side->rec_first[k + 1] - side->rec_first[k];
      if (n_rec > 0xffffffffull) return fail(c, CABAC_HIP_ERR_INVALID, "rec_first: a run longer than 2^32 - 1 records");
      uint32_t at = 0;
      for (uint32_t t = cand_first[k]; side->tu_at && t < cand_first[k + 1]; t++) {
        if (side->tu_at[t] < at) return fail(c, CABAC_HIP_ERR_INVALID, "tu_at decreases inside a candidate");
        if (side->tu_at[t] > n_rec) return fail(c, CABAC_HIP_ERR_INVALID, "tu_at exceeds the candidate's run length");
        at = side->tu_at[t];
      }
      for (uint64_t i = side->rec_first[k]; i < side->rec_first[k + 1]; i++) {
        const uint32_t id = side->records[i] & CABAC_REC_ID_MASK;
        if (id >= CABAC_NUM_CONTEXTS && id < CABAC_REC_ALIGN) {
          char buf[160];
          snprintf(buf, sizeof buf, "bad side record: candidate %u, record %llu of its run (id 0x%x)", k,
                   (unsigned long long)(i - side->rec_first[k]), id);
          return fail(c, CABAC_HIP_ERR_INVALID, buf);
        }
      }
    }
  }
  uint64_t record_bound = 0;
  if (hp)  // what cabac_hip_search_plan.h refuses on top
    if (int bad = check_search_plan_host(c, n_cand, cand_first, tus, *hp, n_coeff_total, &record_bound)) return bad;
  if (n_cand == 0 && n_group == 0) return CABAC_HIP_OK;
  DeviceGuard g(c->device);
  int rc;
  Stage st{c};
  if ((rc = cs.stage(st, state, rate, n_tu ? n_coeff_total * size_t(coeff_bytes) : 0))) return rc;
  SearchStage ss{};
  ss.group_first = st.put(kSearchInGroupFirst, size_t(n_group) + 1, group_first);
  ss.out_set = st.opt(kSearchInOutSet, n_group, group_out_set);
  ss.dist = st.opt(kSearchInDist, n_cand, dist);
  ss.pick = st.room<uint32_t>(kSearchOutPick, n_group);
  ss.cost = st.room<uint64_t>(kSearchOutCost, n_group);
  const uint16_t *d_side = nullptr;
  const uint64_t *d_rec_first = nullptr;
  const uint32_t *d_side_at = nullptr;
  if (side) {
    d_side = st.put(kSearchInRecords, side->n_records_total, side->records);
    d_rec_first = st.put(kSearchInRecFirst, size_t(n_cand) + 1, side->rec_first);
    d_side_at = st.opt(kSearchInTuAt, n_tu, side->tu_at);
  }
  if (st.rc) return st.rc;
  if (hp)
    rc = search_plan_stage_and_run(cs, ss, n_group, *hp, record_bound, lambda_q16);
  else if (side)
    rc = cabac_hip_search_unit_round_device(c, n_group, ss.group_first, n_cand, cs.d_first, cs.d_tu, cs.d_coeff, coeff_bytes, cs.d_state, cs.d_rate,
                                            cs.d_set, d_rec_first, d_side, d_side_at, ss.out_set, ss.dist, lambda_q16, cs.d_bits, ss.pick,
                                            ss.cost, cs.d_tu_bits, cs.d_info, nullptr);
  else
    rc = cabac_hip_search_round_device(c, n_group, ss.group_first, n_cand, cs.d_first, cs.d_tu, cs.d_coeff, coeff_bytes, cs.d_state, cs.d_rate,
                                       cs.d_set, ss.out_set, ss.dist, lambda_q16, cs.d_bits, ss.pick, ss.cost, cs.d_tu_bits, cs.d_info);
  if (rc) return rc;
  if ((rc = cs.fetch(frac_bits, tu_frac_bits))) return rc;
  HIP_TRY(c, down(c, pick, ss.pick, size_t(n_group) * sizeof(uint32_t)));
  HIP_TRY(c, down(c, cost, ss.cost, size_t(n_group) * sizeof(uint64_t)));
  HIP_TRY(c, wait_stream(c, c->stream));
  // the written sets: those of the groups that picked a candidate
  if (group_out_set && n_cand) {
    for (uint32_t k = 0; k < n_group; k++) {
      const uint32_t o = group_out_set[k];
      if (o == CABAC_SEARCH_NO_SET || pick[k] == CABAC_SEARCH_NONE) continue;
      const size_t at = size_t(o) * CABAC_NUM_CONTEXTS;
      HIP_TRY(c, down(c, state + at, cs.d_state + at, CABAC_NUM_CONTEXTS * sizeof(uint32_t)));
      HIP_TRY(c, down(c, rate + at, cs.d_rate + at, CABAC_NUM_CONTEXTS));
    }
    HIP_TRY(c, wait_stream(c, c->stream));
  }
  if (!hp) return cs.info_status(tu_info, true);
  // the plan's info words: a block without records stops its candidate only where it is coded (see flags[])
  (void)cs.info_status(tu_info, false);
  return search_plan_fetch(c, n_cand, *hp);
}

int cabac_hip_search_round_batch(cabac_hip_ctx *c, uint32_t n_group, const uint32_t *group_first, uint32_t n_cand,
                                 const uint32_t *cand_first, const cabac_tu_desc *tus, const void *coeff, int coeff_bytes,
                                 uint64_t n_coeff_total, uint32_t *state, uint8_t *rate, uint32_t n_sets, const uint32_t *set,
                                 const uint32_t *group_out_set, const uint64_t *dist, uint64_t lambda_q16, uint64_t *frac_bits,
                                 uint32_t *pick, uint64_t *cost, uint64_t *tu_frac_bits, uint32_t *tu_info) {
  return search_round_batch_impl(c, n_group, group_first, n_cand, cand_first, tus, coeff, coeff_bytes, n_coeff_total, state, rate,
                                 n_sets, set, group_out_set, dist, lambda_q16, frac_bits, pick, cost, tu_frac_bits, tu_info, nullptr);
}

// ---- search rounds over candidates with side records (declared in cabac_hip_search_unit.h) -------------------------------------
int cabac_hip_estimate_unit_device(cabac_hip_ctx *c, uint32_t n_cand, const uint32_t *d_cand_first, const cabac_tu_desc *d_tu,
                                   const void *d_coeff, int coeff_bytes, const uint32_t *d_state, const uint8_t *d_rate,
                                   const uint32_t *d_set, const uint64_t *d_rec_first, const uint16_t *d_records,
                                   const uint32_t *d_tu_at, uint64_t *d_frac_bits, uint64_t *d_tu_frac_bits, uint32_t *d_tu_info,
                                   uint32_t *d_flags, const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate) {
  if (!c || (n_cand && (!d_cand_first || !d_tu || !d_coeff || !d_state || !d_rate || !d_set || !d_rec_first || !d_frac_bits ||
                        (d_out_set && (!d_out_state || !d_out_rate)))))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (coeff_bytes != 4 && coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (n_cand == 0) return CABAC_HIP_OK;
  DeviceGuard g(c->device);
  if (int rc = ensure(c, kEstScratch, cabac::residual_estimate_scratch_bytes(n_cand))) return rc;
  return TIMED_LAUNCH(c, 19, cabac::launch_unit_estimate(c->stream, n_cand, nullptr, n_cand, d_cand_first, d_tu, d_coeff, coeff_bytes, d_state, d_rate,
                                                         d_set, d_rec_first, d_records, d_tu_at, d_out_set, d_out_state, d_out_rate, d_frac_bits,
                                                         d_tu_frac_bits, d_tu_info, d_flags, c->d_buf[kEstScratch]));
}

int cabac_hip_search_unit_round_device(cabac_hip_ctx *c, uint32_t n_group, const uint32_t *d_group_first, uint32_t n_cand,
                                       const uint32_t *d_cand_first, const cabac_tu_desc *d_tu, const void *d_coeff, int coeff_bytes,
                                       uint32_t *d_state, uint8_t *d_rate, const uint32_t *d_set, const uint64_t *d_rec_first,
                                       const uint16_t *d_records, const uint32_t *d_tu_at, const uint32_t *d_group_out_set,
                                       const uint64_t *d_dist, uint64_t lambda_q16, uint64_t *d_frac_bits, uint32_t *d_pick,
                                       uint64_t *d_cost, uint64_t *d_tu_frac_bits, uint32_t *d_tu_info, uint32_t *d_flags) {
  if (!c || (n_cand && (!d_cand_first || !d_tu || !d_coeff || !d_state || !d_rate || !d_set || !d_rec_first || !d_frac_bits)) ||
      (n_group && (!d_group_first || !d_pick || !d_cost)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (coeff_bytes != 4 && coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (n_cand == 0 && n_group == 0) return CABAC_HIP_OK;
  DeviceGuard g(c->device);
  if (int rc = ensure(c, kEstScratch, cabac::residual_estimate_scratch_bytes(std::max(n_cand, n_group)))) return rc;
  c->timed = false;  // three brackets: read them with cabac_hip_profile_read
  // estimate: every candidate's expanded string from its start set; no set is written
  Bracket br = bracket_for(c, 20);
  HIP_TRY(c, hipEventRecord(br.a, c->stream));
  HIP_TRY(c, cabac::launch_unit_estimate(c->stream, n_cand, nullptr, n_cand, d_cand_first, d_tu, d_coeff, coeff_bytes, d_state, d_rate,
                                         d_set, d_rec_first, d_records, d_tu_at, nullptr, nullptr, nullptr, d_frac_bits, d_tu_frac_bits,
                                         d_tu_info, d_flags, c->d_buf[kEstScratch]));
  HIP_TRY(c, hipEventRecord(br.b, c->stream));
  if (n_group == 0) return CABAC_HIP_OK;
  // select: the kernel of cabac_hip_search_select_device, unchanged
  br = bracket_for(c, 21);
  HIP_TRY(c, hipEventRecord(br.a, c->stream));
  HIP_TRY(c, cabac::launch_search_select(c->stream, n_group, n_cand, d_group_first, d_frac_bits, d_dist, lambda_q16, d_pick, d_cost));
  HIP_TRY(c, hipEventRecord(br.b, c->stream));
  // commit: the picked candidates walked once more with their side records (d_pick is the index list)
  br = bracket_for(c, 22);
  HIP_TRY(c, hipEventRecord(br.a, c->stream));
  if (d_group_out_set && n_cand)
    HIP_TRY(c, cabac::launch_unit_estimate(c->stream, n_group, d_pick, n_cand, d_cand_first, d_tu, d_coeff, coeff_bytes, d_state, d_rate,
                                           d_set, d_rec_first, d_records, d_tu_at, d_group_out_set, d_state, d_rate, nullptr, nullptr,
                                           nullptr, nullptr, c->d_buf[kEstScratch]));
  HIP_TRY(c, hipEventRecord(br.b, c->stream));
  return CABAC_HIP_OK;
}

int cabac_hip_search_unit_round_batch(cabac_hip_ctx *c, uint32_t n_group, const uint32_t *group_first, uint32_t n_cand,
                                      const uint32_t *cand_first, const cabac_tu_desc *tus, const void *coeff, int coeff_bytes,
                                      uint64_t n_coeff_total, uint32_t *state, uint8_t *rate, uint32_t n_sets, const uint32_t *set,
                                      const uint16_t *records, uint64_t n_records_total, const uint64_t *rec_first,
                                      const uint32_t *tu_at, const uint32_t *group_out_set, const uint64_t *dist, uint64_t lambda_q16,
                                      uint64_t *frac_bits, uint32_t *pick, uint64_t *cost, uint64_t *tu_frac_bits, uint32_t *tu_info) {
  const HostSide side{records, n_records_total, rec_first, tu_at};
  return search_round_batch_impl(c, n_group, group_first, n_cand, cand_first, tus, coeff, coeff_bytes, n_coeff_total, state, rate,
                                 n_sets, set, group_out_set, dist, lambda_q16, frac_bits, pick, cost, tu_frac_bits, tu_info, &side);
}

// ---- search rounds over plans (declared in cabac_hip_search_plan.h; kernels in cabac_plan_search.hip) ---------------------------
namespace {
// sizes pass, count walk, scan, emit walk: the resolved form of every candidate.  d_flags: never null here
int resolve_plan_impl(cabac_hip_ctx *c, uint32_t n_cand, const uint32_t *d_cand_first, const uint64_t *d_ent_first, const uint32_t *d_plan,
                      const uint32_t *d_values_in, uint32_t n_tu, const cabac_tu_desc *d_tu, const uint32_t *d_tu_at,
                      const uint32_t *d_tu_guard, const void *d_coeff, int coeff_bytes, uint64_t *d_rec_first, uint16_t *d_records,
                      uint64_t record_capacity, uint32_t *d_tu_at_out, cabac_tu_desc *d_tu_out, uint32_t *d_values_out,
                      uint32_t *d_tu_info, uint32_t *d_flags, uint64_t *d_total) {
  int rc;
  const size_t n_blk = n_tu ? n_tu : 1;
  if ((rc = ensure(c, kSpCnt, 2 * n_blk * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, kResidualScratch, cabac::residual_scratch_bytes(n_tu)))) return rc;
  uint32_t *d_cnt = static_cast<uint32_t *>(c->d_buf[kSpCnt]), *d_info = d_cnt + n_blk;
  uint32_t *cnt = static_cast<uint32_t *>(c->d_buf[kPsCnt]);
  const cabac::PlanResolveIn in{n_cand, d_cand_first, d_ent_first, d_plan, d_values_in, n_tu, d_tu, d_tu_at, d_tu_guard, d_info};
  const cabac::PlanResolveOut out{d_rec_first, d_records, d_tu_at_out, d_tu_out, d_values_out, d_tu_info};
  {  // info words of ALL blocks: they do not depend on the guards, the guards depend on them
    Timed t(c, 5);
    HIP_TRY(c, cabac::launch_residual(c->stream, n_tu, d_tu, d_coeff, coeff_bytes, nullptr, d_cnt, d_info, nullptr, c->d_buf[kResidualScratch]));
  }
  {
    Timed t(c, 29);
    HIP_TRY(c, cabac::launch_plan_resolve_count(c->stream, in, cnt, d_flags));
    HIP_TRY(c, cabac::launch_plan_resolve_scan(c->stream, n_cand, cnt, d_flags, record_capacity, d_rec_first, d_total));
    HIP_TRY(c, cabac::launch_plan_resolve_emit(c->stream, in, cnt, d_flags, out));
  }
  return CABAC_HIP_OK;
}

// the pointers a resolve needs, for both device forms
bool resolve_plan_null(uint32_t n_cand, const uint32_t *d_cand_first, const uint64_t *d_ent_first, uint32_t n_tu, const cabac_tu_desc *d_tu,
                       const void *d_coeff, uint64_t *d_rec_first, uint16_t *d_records, uint64_t record_capacity, uint32_t *d_tu_at_out,
                       cabac_tu_desc *d_tu_out) {
  return !d_rec_first || (n_cand && (!d_cand_first || !d_ent_first)) || (n_tu && (!d_tu || !d_coeff || !d_tu_at_out || !d_tu_out)) ||
         (record_capacity && !d_records) || (n_tu && d_tu_out == d_tu);
}
}  // namespace

int cabac_hip_resolve_plan_device(cabac_hip_ctx *c, uint32_t n_cand, const uint32_t *d_cand_first, const uint64_t *d_ent_first,
                                  const uint32_t *d_plan, const uint32_t *d_values_in, uint32_t n_tu, const cabac_tu_desc *d_tu,
                                  const uint32_t *d_tu_at, const uint32_t *d_tu_guard, const void *d_coeff, int coeff_bytes,
                                  uint64_t *d_rec_first, uint16_t *d_records, uint64_t record_capacity, uint32_t *d_tu_at_out,
                                  cabac_tu_desc *d_tu_out, uint32_t *d_values_out, uint32_t *d_tu_info, uint32_t *d_flags,
                                  uint64_t *d_total) {
  if (!c || (n_cand && !d_flags) ||
      resolve_plan_null(n_cand, d_cand_first, d_ent_first, n_tu, d_tu, d_coeff, d_rec_first, d_records, record_capacity, d_tu_at_out, d_tu_out))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (coeff_bytes != 4 && coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (n_cand == 0 && n_tu) return fail(c, CABAC_HIP_ERR_INVALID, "blocks without a candidate");
  DeviceGuard g(c->device);
  if (int rc = ensure(c, kPsCnt, size_t(n_cand ? n_cand : 1) * sizeof(uint32_t))) return rc;
  c->timed = false;
  return resolve_plan_impl(c, n_cand, d_cand_first, d_ent_first, d_plan, d_values_in, n_tu, d_tu, d_tu_at, d_tu_guard, d_coeff, coeff_bytes,
                           d_rec_first, d_records, record_capacity, d_tu_at_out, d_tu_out, d_values_out, d_tu_info, d_flags, d_total);
}

int cabac_hip_search_plan_round_device(cabac_hip_ctx *c, uint32_t n_group, const uint32_t *d_group_first, uint32_t n_cand,
                                       const uint32_t *d_cand_first, uint32_t n_tu, const cabac_tu_desc *d_tu, const void *d_coeff,
                                       int coeff_bytes, uint32_t *d_state, uint8_t *d_rate, const uint32_t *d_set,
                                       const uint64_t *d_ent_first, const uint32_t *d_plan, const uint32_t *d_values_in,
                                       const uint32_t *d_tu_at, const uint32_t *d_tu_guard, const uint32_t *d_group_out_set,
                                       const uint64_t *d_dist, uint64_t lambda_q16, uint64_t *d_frac_bits, uint32_t *d_pick,
                                       uint64_t *d_cost, uint64_t *d_tu_frac_bits, uint32_t *d_tu_info, uint32_t *d_flags,
                                       uint64_t *d_rec_first, uint16_t *d_records, uint64_t record_capacity, uint32_t *d_tu_at_out,
                                       cabac_tu_desc *d_tu_out, uint32_t *d_values_out, uint64_t *d_total) {
  if (!c || (n_cand && (!d_state || !d_rate || !d_set || !d_frac_bits)) || (n_group && (!d_group_first || !d_pick || !d_cost)) ||
      resolve_plan_null(n_cand, d_cand_first, d_ent_first, n_tu, d_tu, d_coeff, d_rec_first, d_records, record_capacity, d_tu_at_out, d_tu_out))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (coeff_bytes != 4 && coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (n_cand == 0 && n_tu) return fail(c, CABAC_HIP_ERR_INVALID, "blocks without a candidate");
  if (n_cand == 0 && n_group == 0) return CABAC_HIP_OK;
  DeviceGuard g(c->device);
  int rc;
  if ((rc = ensure(c, kEstScratch, cabac::residual_estimate_scratch_bytes(std::max(n_cand, n_group))))) return rc;
  if ((rc = ensure(c, kPsCnt, 2 * size_t(n_cand ? n_cand : 1) * sizeof(uint32_t)))) return rc;
  uint32_t *flags = d_flags ? d_flags : static_cast<uint32_t *>(c->d_buf[kPsCnt]) + (n_cand ? n_cand : 1);
  c->timed = false;  // several brackets: read them with cabac_hip_profile_read
  if ((rc = resolve_plan_impl(c, n_cand, d_cand_first, d_ent_first, d_plan, d_values_in, n_tu, d_tu, d_tu_at, d_tu_guard, d_coeff,
                              coeff_bytes, d_rec_first, d_records, record_capacity, d_tu_at_out, d_tu_out, d_values_out, d_tu_info, flags,
                              d_total)))
    return rc;
  {  // estimate: every candidate's resolved form from its start set; the info words and the flags stay the resolve's
    Timed t(c, 20);
    HIP_TRY(c, cabac::launch_unit_estimate(c->stream, n_cand, nullptr, n_cand, d_cand_first, d_tu_out, d_coeff, coeff_bytes, d_state, d_rate,
                                           d_set, d_rec_first, d_records, d_tu_at_out, nullptr, nullptr, nullptr, d_frac_bits,
                                           d_tu_frac_bits, nullptr, nullptr, c->d_buf[kEstScratch]));
  }
  {  // select, in front of it the cost of the flagged candidates
    Timed t(c, 21);
    HIP_TRY(c, cabac::launch_plan_flag_cost(c->stream, n_cand, flags, d_frac_bits));
    if (n_group)
      HIP_TRY(c, cabac::launch_search_select(c->stream, n_group, n_cand, d_group_first, d_frac_bits, d_dist, lambda_q16, d_pick, d_cost));
  }
  {  // commit: the picked candidates walked once more in their resolved form (d_pick is the index list)
    Timed t(c, 22);
    if (n_group && d_group_out_set && n_cand)
      HIP_TRY(c, cabac::launch_unit_estimate(c->stream, n_group, d_pick, n_cand, d_cand_first, d_tu_out, d_coeff, coeff_bytes, d_state,
                                             d_rate, d_set, d_rec_first, d_records, d_tu_at_out, d_group_out_set, d_state, d_rate, nullptr,
                                             nullptr, nullptr, nullptr, c->d_buf[kEstScratch]));
  }
  return CABAC_HIP_OK;
}

int cabac_hip_search_plan_round_batch(cabac_hip_ctx *c, uint32_t n_group, const uint32_t *group_first, uint32_t n_cand,
                                      const uint32_t *cand_first, const cabac_tu_desc *tus, const void *coeff, int coeff_bytes,
                                      uint64_t n_coeff_total, uint32_t *state, uint8_t *rate, uint32_t n_sets, const uint32_t *set,
                                      const uint32_t *plan, const uint32_t *values_in, uint64_t n_entries_total,
                                      const uint64_t *ent_first, const uint32_t *tu_at, const uint32_t *tu_guard,
                                      const uint32_t *group_out_set, const uint64_t *dist, uint64_t lambda_q16, uint64_t *frac_bits,
                                      uint32_t *pick, uint64_t *cost, uint64_t *tu_frac_bits, uint32_t *tu_info, uint32_t *flags,
                                      uint32_t *values_out) {
  const HostPlan hp{plan, values_in, n_entries_total, ent_first, tu_at, tu_guard, flags, values_out};
  return search_round_batch_impl(c, n_group, group_first, n_cand, cand_first, tus, coeff, coeff_bytes, n_coeff_total, state, rate,
                                 n_sets, set, group_out_set, dist, lambda_q16, frac_bits, pick, cost, tu_frac_bits, tu_info, nullptr, &hp);
}

// ---- the winner log (declared in cabac_hip_search_emit.h; kernels in cabac_search_emit.hip) -------------------------------------
namespace {
void log_free(cabac_search_log *log) {
  void *p[] = {log->a.counters, log->a.entries, log->a.records, log->a.tu, log->a.tu_at, log->a.coeff, log->a.chain_rec, log->a.chain_tu,
               log->a.mark_rec, log->a.mark_tu};
  for (void *q : p)
    if (q) (void)device_free(log->ctx, q);
  delete log;
}
}  // namespace

int cabac_hip_search_log_create(cabac_hip_ctx *c, uint32_t n_chain, uint32_t entry_capacity, uint64_t record_capacity,
                                uint32_t tu_capacity, uint64_t coeff_capacity, int coeff_bytes, cabac_search_log **out) {
  if (!c || !out) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  *out = nullptr;
  if (n_chain == 0) return fail(c, CABAC_HIP_ERR_INVALID, "a log needs at least one chain");
  if (coeff_bytes != 4 && coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (record_capacity > (uint64_t(1) << 60) || coeff_capacity > (uint64_t(1) << 60)) return fail(c, CABAC_HIP_ERR_INVALID, "capacity");
  DeviceGuard g(c->device);
  cabac_search_log *log = new (std::nothrow) cabac_search_log;
  if (!log) return fail(c, CABAC_HIP_ERR_NOMEM, "out of host memory");
  log->ctx = c;
  log->coeff_bytes = coeff_bytes;
  cabac::SearchLogArrays &a = log->a;
  a.n_chain = n_chain;
  a.entry_cap = entry_capacity;
  a.record_cap = record_capacity;
  a.tu_cap = tu_capacity;
  a.coeff_cap = coeff_capacity;
  auto alloc = [c](auto **p, size_t bytes) { return device_alloc(c, reinterpret_cast<void **>(p), bytes + 16) == hipSuccess; };  // + 16: never empty
  if (!alloc(&a.counters, sizeof(cabac_search_log_counters)) || !alloc(&a.entries, size_t(entry_capacity) * sizeof(cabac_search_log_entry)) ||
      !alloc(&a.records, record_capacity * sizeof(uint16_t)) || !alloc(&a.tu, size_t(tu_capacity) * sizeof(cabac_tu_desc)) ||
      !alloc(&a.tu_at, size_t(tu_capacity) * sizeof(uint32_t)) || !alloc(&a.coeff, coeff_capacity * size_t(coeff_bytes)) ||
      !alloc(&a.chain_rec, size_t(n_chain) * sizeof(uint32_t)) || !alloc(&a.chain_tu, size_t(n_chain) * sizeof(uint32_t)) ||
      !alloc(&a.mark_rec, size_t(n_chain) * sizeof(uint32_t)) || !alloc(&a.mark_tu, size_t(n_chain) * sizeof(uint32_t))) {
    (void)hipGetLastError();
    log_free(log);
    return fail(c, CABAC_HIP_ERR_NOMEM, "hipMalloc failed");
  }
  hipError_t e = cabac::launch_search_log_reset(c->stream, a);
  if (e != hipSuccess) {
    log_free(log);
    return fail_hip(c, e, "cabac_hip_search_log_create");
  }
  c->logs.push_back(log);
  *out = log;
  return CABAC_HIP_OK;
}

int cabac_hip_search_log_destroy(cabac_search_log *log) {
  if (!log) return CABAC_HIP_OK;
  cabac_hip_ctx *c = log->ctx;
  DeviceGuard g(c->device);
  (void)wait_stream(c, c->stream);  // what is queued may still read or write the log
  c->logs.erase(std::remove(c->logs.begin(), c->logs.end(), log), c->logs.end());
  log_free(log);
  return CABAC_HIP_OK;
}

int cabac_hip_search_log_reset_device(cabac_search_log *log) {
  if (!log) return CABAC_HIP_ERR_INVALID;
  cabac_hip_ctx *c = log->ctx;
  DeviceGuard g(c->device);
  HIP_TRY(c, cabac::launch_search_log_reset(c->stream, log->a));
  return CABAC_HIP_OK;
}

int cabac_hip_search_log_append_device(cabac_search_log *log, uint32_t n_group, const uint32_t *d_pick, const uint32_t *d_group_chain,
                                       uint32_t n_cand, const uint32_t *d_cand_first, const cabac_tu_desc *d_tu, const void *d_coeff,
                                       int coeff_bytes, const uint64_t *d_rec_first, const uint16_t *d_records, const uint32_t *d_tu_at) {
  if (!log) return CABAC_HIP_ERR_INVALID;
  cabac_hip_ctx *c = log->ctx;
  if (n_group && (!d_pick || !d_group_chain || !d_cand_first || !d_rec_first)) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (coeff_bytes != log->coeff_bytes) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes is not the log's");
  if (n_group == 0) return CABAC_HIP_OK;
  DeviceGuard g(c->device);
  if (int rc = ensure(c, kLogScratch, cabac::search_log_scratch_bytes(n_group))) return rc;
  c->timed = false;
  Timed t(c, 23);
  HIP_TRY(c, cabac::launch_search_log_append(c->stream, log->a, n_group, d_pick, d_group_chain, n_cand, d_cand_first, d_tu, d_coeff,
                                             coeff_bytes, d_rec_first, d_records, d_tu_at, c->d_buf[kLogScratch]));
  return CABAC_HIP_OK;
}

int cabac_hip_search_log_view(const cabac_search_log *log, cabac_search_log_view *view) {
  if (!log || !view) return CABAC_HIP_ERR_INVALID;
  const cabac::SearchLogArrays &a = log->a;
  view->d_counters = a.counters;
  view->d_entries = a.entries;
  view->d_records = a.records;
  view->d_tu = a.tu;
  view->d_tu_at = a.tu_at;
  view->d_coeff = a.coeff;
  view->record_capacity = a.record_cap;
  view->coeff_capacity = a.coeff_cap;
  view->n_chain = a.n_chain;
  view->entry_capacity = a.entry_cap;
  view->tu_capacity = a.tu_cap;
  view->coeff_bytes = log->coeff_bytes;
  return CABAC_HIP_OK;
}

// The emit on a fixed workspace (cabac_hip_workspace.h): the counters stay on the device and every launch is sized from the log's
// capacities; the place pass hands the binariser tu_cap descriptors, the unused ones rejected, and the splice kernels count the
// logged blocks by the device's word.
static int search_log_encode_fixed(cabac_search_log *log, const cabac_substream_desc *d_desc, const PayloadOut &out, uint32_t *d_bin_counts,
                                   const cabac::CtxSets *sets, const Rows *rows) {
  cabac_hip_ctx *c = log->ctx;
  const cabac::SearchLogArrays &a = log->a;
  if (int bad = check_workspace(c, a.n_chain, a.tu_cap, rows != nullptr)) return bad;
  if (a.record_cap > c->ws.log_records)
    return fail(c, CABAC_HIP_ERR_INVALID, "the log's record_capacity exceeds the fixed workspace (log_records)");
  int rc;
  if ((rc = ensure(c, kLogDesc, size_t(a.n_chain) * sizeof(cabac_substream_desc)))) return rc;
  if ((rc = ensure(c, kLogFirst, (size_t(a.n_chain) + 1) * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, kLogRec, (a.record_cap + 8) * sizeof(uint16_t)))) return rc;
  if ((rc = ensure(c, kLogSplice, size_t(a.tu_cap ? a.tu_cap : 1) * sizeof(cabac_splice)))) return rc;
  if ((rc = ensure(c, kPwTu, size_t(a.tu_cap ? a.tu_cap : 1) * sizeof(cabac_tu_desc)))) return rc;
  auto *desc2 = static_cast<cabac_substream_desc *>(c->d_buf[kLogDesc]);
  auto *first = static_cast<uint32_t *>(c->d_buf[kLogFirst]);
  auto *rec = static_cast<uint16_t *>(c->d_buf[kLogRec]);
  auto *splices = static_cast<cabac_splice *>(c->d_buf[kLogSplice]);
  auto *tus = static_cast<cabac_tu_desc *>(c->d_buf[kPwTu]);
  {
    Timed t(c, 24);
    HIP_TRY(c, cabac::launch_search_log_place_fixed(c->stream, a, c->d_ws, d_desc, desc2, first, rec, splices, tus));
  }
  Rows marked{};
  if (rows) marked = Rows{rows->n_level, rows->level_first, rows->d_sync_from, a.mark_rec, a.mark_tu};
  PayloadOut no_info = out;  // (the binariser's words are per descriptor handed over, used or not)
  no_info.d_tu_info = nullptr;
  if ((rc = encode_residual_device_impl(c, a.n_chain, {desc2, rec, first, splices, a.tu_cap, a.tu_cap, tus, a.coeff, log->coeff_bytes}, no_info,
                                        d_bin_counts, sets, rows ? &marked : nullptr, &c->d_ws->log_tu)))
    return rc;
  if (uint32_t *d_tu_info = out.d_tu_info) {  // one word per LOGGED block: the count is the device's
    Timed t(c, 40);
    HIP_TRY(c, cabac::launch_ws_log_info(c->stream, c->d_ws, a.tu_cap, static_cast<uint32_t *>(c->d_buf[kSpCnt]) + (a.tu_cap ? a.tu_cap : 1),
                                         d_tu_info));
  }
  return CABAC_HIP_OK;
}

// sets / rows (may be null, not both): handed on to the spliced encode; a rows call takes the chains' marks as the hand-over pairs
// (its d_sync_at and d_sync_splice are not read)
static int search_log_encode_impl(cabac_search_log *log, const cabac_substream_desc *d_desc, const PayloadOut &out, uint32_t *d_bin_counts,
                                  const cabac::CtxSets *sets, const Rows *rows) {
  if (!log) return CABAC_HIP_ERR_INVALID;
  cabac_hip_ctx *c = log->ctx;
  if (!d_desc || !out.d_payload || !out.d_payload_offsets || !out.d_results) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  const cabac::SearchLogArrays &a = log->a;
  if (c->ws_fixed) return search_log_encode_fixed(log, d_desc, out, d_bin_counts, sets, rows);
  if (!c->h_totals) HIP_TRY(c, pinned_alloc(c, &c->h_totals, 64, hipHostMallocDefault));
  static_assert(sizeof(cabac_search_log_counters) <= 64, "the pinned block of the ctx holds the counters");
  HIP_TRY(c, hipMemcpyAsync(c->h_totals, a.counters, sizeof(cabac_search_log_counters), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, wait_stream(c, c->stream));  // the first wait: the counters size everything below
  const cabac_search_log_counters cnt = *static_cast<const cabac_search_log_counters *>(c->h_totals);
  if (cnt.flags & CABAC_SEARCH_LOG_OVERFLOW) {
    std::string msg = "the log overflowed (an append was dropped):";
    if (cnt.flags & CABAC_SEARCH_LOG_OVER_ENTRIES) msg += " entry_capacity";
    if (cnt.flags & CABAC_SEARCH_LOG_OVER_RECORDS) msg += " record_capacity";
    if (cnt.flags & CABAC_SEARCH_LOG_OVER_BLOCKS) msg += " tu_capacity";
    if (cnt.flags & CABAC_SEARCH_LOG_OVER_COEFFS) msg += " coeff_capacity";
    if (cnt.flags & CABAC_SEARCH_LOG_OVER_CHAIN_RECORDS) msg += " 2^32 - 1 records of one chain";
    return fail(c, CABAC_HIP_ERR_INVALID, msg.c_str());
  }
  if (cnt.n_entry > a.entry_cap || cnt.n_record > a.record_cap || cnt.n_tu > a.tu_cap || cnt.n_coeff > a.coeff_cap)
    return fail(c, CABAC_HIP_ERR_INVALID, "the log's counters are damaged");
  const uint32_t n_entry = (uint32_t)cnt.n_entry, n_tu = (uint32_t)cnt.n_tu;
  int rc;
  if ((rc = ensure(c, kLogDesc, size_t(a.n_chain) * sizeof(cabac_substream_desc)))) return rc;
  if ((rc = ensure(c, kLogFirst, (size_t(a.n_chain) + 1) * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, kLogRec, (cnt.n_record + 8) * sizeof(uint16_t)))) return rc;
  if ((rc = ensure(c, kLogSplice, size_t(n_tu ? n_tu : 1) * sizeof(cabac_splice)))) return rc;
  auto *desc2 = static_cast<cabac_substream_desc *>(c->d_buf[kLogDesc]);
  auto *first = static_cast<uint32_t *>(c->d_buf[kLogFirst]);
  auto *rec = static_cast<uint16_t *>(c->d_buf[kLogRec]);
  auto *splices = static_cast<cabac_splice *>(c->d_buf[kLogSplice]);
  {
    Timed t(c, 24);
    HIP_TRY(c, cabac::launch_search_log_place(c->stream, a, d_desc, n_entry, cnt.n_record, n_tu, desc2, first, rec, splices));
  }
  Rows marked{};
  if (rows) marked = Rows{rows->n_level, rows->level_first, rows->d_sync_from, a.mark_rec, a.mark_tu};
  return encode_residual_device_impl(c, a.n_chain, {desc2, rec, first, splices, n_tu, n_tu, a.tu, a.coeff, log->coeff_bytes}, out, d_bin_counts,
                                     sets, rows ? &marked : nullptr);
}

int cabac_hip_search_log_encode_device(cabac_search_log *log, const cabac_substream_desc *d_desc, uint8_t *d_payload,
                                       uint64_t payload_capacity, uint64_t *d_payload_offsets, cabac_substream_result *d_results,
                                       uint32_t *d_tu_info, uint32_t *d_bin_counts) {
  return search_log_encode_impl(log, d_desc, {d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info}, d_bin_counts, nullptr,
                                nullptr);
}

// ---- context sets and WPP (cabac_hip_ctx_sets.h; the schedule of a WPP call is wpp_device_impl above) ---------------------------
int cabac_hip_encode_sets_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                 uint8_t *d_bytes, cabac_substream_result *d_results, uint32_t n_sets, const uint32_t *d_state,
                                 const uint8_t *d_rate, const uint32_t *d_start_set, const uint32_t *d_out_set, uint32_t *d_out_state,
                                 uint8_t *d_out_rate) {
  if (!c || (n_sub && (!d_desc || !d_records || !d_bytes || !d_results)) ||
      !sets_args_ok(n_sub, n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  const cabac::CtxSets sets{n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate};
  return TIMED_LAUNCH(c, 30, cabac::launch_encode(c->stream, c->enc_variant, n_sub, d_desc, d_records, d_bytes, d_results, 0, &sets));
}

int cabac_hip_decode_sets_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                 const uint8_t *d_bytes, uint8_t *d_bins, cabac_substream_result *d_results, uint32_t n_sets,
                                 const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set,
                                 const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate) {
  if (!c || (n_sub && (!d_desc || !d_records || !d_bytes || !d_bins || !d_results)) ||
      !sets_args_ok(n_sub, n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  const cabac::CtxSets sets{n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate};
  return TIMED_LAUNCH(c, 31, cabac::launch_decode(c->stream, c->dec_variant, n_sub, d_desc, d_records, d_bytes, d_bins, d_results, 0, c->d_select, &sets));
}

int cabac_hip_ctx_advance_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                 uint32_t n_sets, const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set,
                                 const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate, uint32_t *d_flags) {
  if (!c || (n_sub && (!d_desc || !d_records)) ||
      !sets_args_ok(n_sub, n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  const cabac::CtxSets sets{n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate};
  return TIMED_LAUNCH(c, 32, cabac::launch_ctx_advance(c->stream, n_sub, d_desc, d_records, sets, d_flags));
}

// ---- the encoder of the pieces calls (cabac_hip_piece_encoder.h) -----------------------------------------------------------------
// Setting 0: the lane-serial encoder from this many substreams in the call, the in-wave one below.  Measured (tools/bench_piece_encoder.py,
// profiles/piece_encoder.json: four pieces of substreams of 16 384 records, the first N of the 1080p batch, setting 4 / setting 7):
// N = 256 1.563 / 0.500 ms, 1 024 1.575 / 0.568, 2 048 1.691 / 0.575, 4 096 1.636 / 0.602 — 7 never loses, so the threshold is 0
// and setting 0 is setting 7 on every batch measured.  Results never depend on it.
static constexpr uint32_t kPieceEncoderV7From = 0;

static int piece_encoder_for(const cabac_hip_ctx *c, uint32_t n_sub) {
  if (c->piece_encoder != 0) return c->piece_encoder;
  return (kPieceEncoderV7From == 0u || n_sub >= kPieceEncoderV7From) ? 7 : 4;
}

int cabac_hip_piece_encoder_set(cabac_hip_ctx *c, int variant) {
  if (!c) return CABAC_HIP_ERR_INVALID;
  if (variant != 4 && variant != 7 && variant != 0) return fail(c, CABAC_HIP_ERR_INVALID, "piece encoder: 4, 7 or 0");
  c->piece_encoder = variant;
  return CABAC_HIP_OK;
}

int cabac_hip_piece_encoder_get(const cabac_hip_ctx *c) { return c ? c->piece_encoder : CABAC_HIP_ERR_INVALID; }

// ---- the bin codec in pieces (cabac_hip_pieces.h): not dispatched, one geometry each ----------------------------------------------
int cabac_hip_encode_pieces_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                   uint8_t *d_bytes, cabac_substream_result *d_results, uint32_t n_sets, const uint32_t *d_state,
                                   const uint8_t *d_rate, const uint32_t *d_start_set, const uint32_t *d_out_set, uint32_t *d_out_state,
                                   uint8_t *d_out_rate, const cabac_coder_state *d_coder_in, cabac_coder_state *d_coder_out) {
  if (!c || (n_sub && (!d_desc || !d_records || !d_bytes || !d_results)) ||
      !sets_args_ok(n_sub, n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (n_sub == 0) return CABAC_HIP_OK;
  DeviceGuard g(c->device);
  const cabac::CtxPieces pieces{{n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate}, d_coder_in, d_coder_out};
  return TIMED_LAUNCH(c, 48, cabac::launch_encode_pieces(c->stream, n_sub, d_desc, d_records, d_bytes, d_results, pieces,
                                                         piece_encoder_for(c, n_sub)));
}

int cabac_hip_decode_pieces_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                   const uint8_t *d_bytes, uint8_t *d_bins, cabac_substream_result *d_results, uint32_t n_sets,
                                   const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set,
                                   const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate,
                                   const cabac_coder_state *d_coder_in, cabac_coder_state *d_coder_out) {
  if (!c || (n_sub && (!d_desc || !d_records || !d_bytes || !d_bins || !d_results)) ||
      !sets_args_ok(n_sub, n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (n_sub == 0) return CABAC_HIP_OK;
  DeviceGuard g(c->device);
  const cabac::CtxPieces pieces{{n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate}, d_coder_in, d_coder_out};
  return TIMED_LAUNCH(c, 49, cabac::launch_decode_pieces(c->stream, n_sub, d_desc, d_records, d_bytes, d_bins, d_results, pieces));
}

int cabac_hip_encode_wpp_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                uint8_t *d_bytes, cabac_substream_result *d_results, uint32_t n_level, const uint32_t *level_first,
                                const uint32_t *d_sync_from, const uint32_t *d_sync_at) {
  return wpp_device_impl(c, false, n_sub, d_desc, d_records, d_bytes, nullptr, d_results, n_level, level_first, d_sync_from, d_sync_at);
}

int cabac_hip_decode_wpp_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                const uint8_t *d_bytes, uint8_t *d_bins, cabac_substream_result *d_results, uint32_t n_level,
                                const uint32_t *level_first, const uint32_t *d_sync_from, const uint32_t *d_sync_at) {
  return wpp_device_impl(c, true, n_sub, d_desc, d_records, const_cast<uint8_t *>(d_bytes), d_bins, d_results, n_level, level_first,
                         d_sync_from, d_sync_at);
}

// host-pointer forms: one chunk (chunks would cut links), everything on the ctx stream
static int wpp_batch_impl(cabac_hip_ctx *c, bool decode, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                          uint64_t n_records_total, uint8_t *bytes, uint64_t bytes_total, uint8_t *bins, cabac_substream_result *results,
                          uint32_t n_level, const uint32_t *level_first, const uint32_t *sync_from, const uint32_t *sync_at) {
  if (!c || (n_sub && (!desc || !results || !bytes || (n_records_total && !records) || (decode && n_records_total && !bins) ||
                       !sync_from || !sync_at)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (n_sub == 0) return CABAC_HIP_OK;
  int rc = check_desc_host(c, n_sub, desc, n_records_total, bytes_total);
  if (rc) return rc;
  if ((rc = check_levels(c, n_sub, n_level, level_first))) return rc;
  if ((rc = check_links_host(c, n_sub, n_level, level_first, sync_from))) return rc;
  DeviceGuard g(c->device);
  if ((rc = pipe_init(c))) return rc;
  const size_t res_bytes = size_t(n_sub) * sizeof(cabac_substream_result);
  if ((rc = ensure_pinned(c, 0, res_bytes))) return rc;
  auto *h_res = static_cast<cabac_substream_result *>(c->h_pin[0]);
  hipStream_t stream = c->stream;
  HIP_TRY(c, wait_stream(c, stream));
  Stage st{c, true, stream};
  auto *d_desc = st.put(kDesc, n_sub, desc);
  auto *d_rec = st.put(kRecords, n_records_total, records);
  const Rows d_rows = stage_rows(st, n_sub, Rows{n_level, level_first, sync_from, sync_at}, false);
  // decode: the bytes go up; encode: the whole range goes back, so what no substream writes stays zero
  auto *d_slots = static_cast<uint8_t *>(st.bytes(kBytes, bytes_total + 4, bytes, decode ? bytes_total : 0));
  auto *d_res = st.room<cabac_substream_result>(kResults, n_sub);
  auto *d_bins = decode ? st.room<uint8_t>(kBins, n_records_total + 8) : nullptr;
  if (st.rc) return st.rc;
  if (!decode) HIP_TRY(c, hipMemsetAsync(d_slots, 0, bytes_total, stream));
  if ((rc = wpp_device_impl(c, decode, n_sub, d_desc, d_rec, d_slots, d_bins, d_res, n_level, level_first, d_rows.d_sync_from, d_rows.d_sync_at)))
    return rc;
  HIP_TRY(c, hipMemcpyAsync(h_res, d_res, res_bytes, hipMemcpyDeviceToHost, stream));
  if ((rc = d2h(c, decode ? bins : bytes, decode ? d_bins : d_slots, decode ? n_records_total : bytes_total, stream))) return rc;
  if ((rc = d2h_drain(c))) return rc;
  HIP_TRY(c, wait_stream(c, stream));
  return flags_status(c, n_sub, h_res, results, "substream flag set (see results[].flags)");
}

int cabac_hip_encode_wpp_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                               uint64_t n_records_total, uint8_t *bytes, uint64_t bytes_total, cabac_substream_result *results,
                               uint32_t n_level, const uint32_t *level_first, const uint32_t *sync_from, const uint32_t *sync_at) {
  return host_call_exit(c, wpp_batch_impl(c, false, n_sub, desc, records, n_records_total, bytes, bytes_total, nullptr, results, n_level,
                                          level_first, sync_from, sync_at));
}

int cabac_hip_decode_wpp_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                               uint64_t n_records_total, const uint8_t *bytes, uint64_t bytes_total, uint8_t *bins,
                               cabac_substream_result *results, uint32_t n_level, const uint32_t *level_first,
                               const uint32_t *sync_from, const uint32_t *sync_at) {
  return host_call_exit(c, wpp_batch_impl(c, true, n_sub, desc, records, n_records_total, const_cast<uint8_t *>(bytes), bytes_total, bins,
                                          results, n_level, level_first, sync_from, sync_at));
}

// ---- plan rows (cabac_hip_plan_rows.h): the plan parse and the plan write from and into context sets, and in WPP rows ----------
int cabac_hip_plan_parse_sets_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint8_t *d_bytes,
                                     const uint32_t *d_tile_first, const cabac_tu_desc *d_tu, const uint32_t *d_tu_at,
                                     const uint32_t *d_tu_guard, const uint32_t *d_plan, void *d_coeff, int coeff_bytes,
                                     uint32_t *d_values, uint32_t *d_tu_info, cabac_substream_result *d_results, uint32_t n_sets,
                                     const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set,
                                     const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate, const uint32_t *d_out_at) {
  const cabac::ParseIn in{d_desc, d_bytes, d_tile_first, d_tu, d_coeff, coeff_bytes, d_tu_info, d_results, d_tu_at, d_tu_guard, d_plan, d_values};
  const cabac::CtxSets sets{n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate};
  return PARSE_DEVICE_CALL(c, n_sub, in, sets_args_ok(n_sub, n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate), 34,
                           cabac::launch_plan_parse_sets(c->stream, n_sub, in, sets, d_out_at, n_sets, 0xFFFFFFFFu));
}

// ---- the plan parse in pieces (cabac_hip_plan_resume.h): the sets form's checks, one coder state per substream in and out --------
int cabac_hip_plan_resume_parse_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint8_t *d_bytes,
                                       const uint32_t *d_tile_first, const cabac_tu_desc *d_tu, const uint32_t *d_tu_at,
                                       const uint32_t *d_tu_guard, const uint32_t *d_plan, void *d_coeff, int coeff_bytes,
                                       uint32_t *d_values, uint32_t *d_tu_info, cabac_substream_result *d_results, uint32_t n_sets,
                                       const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set,
                                       const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate, const void *d_coder_in,
                                       void *d_coder_out) {
  const cabac::ParseIn in{d_desc, d_bytes, d_tile_first, d_tu, d_coeff, coeff_bytes, d_tu_info, d_results, d_tu_at, d_tu_guard, d_plan, d_values};
  const cabac::CtxPieces pieces{{n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate},
                                static_cast<const cabac_coder_state *>(d_coder_in), static_cast<cabac_coder_state *>(d_coder_out)};
  return PARSE_DEVICE_CALL(c, n_sub, in, sets_args_ok(n_sub, n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate), 50,
                           cabac::launch_plan_parse_pieces(c->stream, n_sub, in, pieces));
}

int cabac_hip_plan_parse_rows_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint8_t *d_bytes,
                                     const uint32_t *d_tile_first, const cabac_tu_desc *d_tu, const uint32_t *d_tu_at,
                                     const uint32_t *d_tu_guard, const uint32_t *d_plan, void *d_coeff, int coeff_bytes,
                                     uint32_t *d_values, uint32_t *d_tu_info, cabac_substream_result *d_results, uint32_t n_level,
                                     const uint32_t *level_first, const uint32_t *d_sync_from, const uint32_t *d_sync_at) {
  return parse_rows_device_impl(c, n_sub, {d_desc, d_bytes, d_tile_first, d_tu, d_coeff, coeff_bytes, d_tu_info, d_results, d_tu_at, d_tu_guard,
                                           d_plan, d_values},
                                Rows{n_level, level_first, d_sync_from, d_sync_at});
}

int cabac_hip_plan_parse_rows_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *bytes,
                                    uint64_t bytes_total, const uint32_t *tile_first, const cabac_tu_desc *tus, const uint32_t *tu_at,
                                    const uint32_t *tu_guard, const uint32_t *plan, uint64_t n_elements_total, void *coeff,
                                    int coeff_bytes, uint64_t n_coeff_total, uint32_t *values, uint32_t *tu_info,
                                    cabac_substream_result *results, uint32_t n_level, const uint32_t *level_first,
                                    const uint32_t *sync_from, const uint32_t *sync_at) {
  const Rows rows{n_level, level_first, sync_from, sync_at};
  return parse_plan_batch_impl(c, n_sub, desc, bytes, bytes_total, tile_first, tus, tu_at, tu_guard, plan, n_elements_total, coeff,
                               coeff_bytes, n_coeff_total, values, tu_info, results, kPlanRules, &rows);
}

int cabac_hip_plan_write_sets_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint32_t *d_plan,
                                     const uint32_t *d_values_in, const uint32_t *d_tile_first, uint32_t n_tu, const cabac_tu_desc *d_tu,
                                     const uint32_t *d_tu_at, const uint32_t *d_tu_guard, const void *d_coeff, int coeff_bytes,
                                     uint8_t *d_payload, uint64_t payload_capacity, uint64_t *d_payload_offsets,
                                     cabac_substream_result *d_results, uint32_t *d_values_out, uint32_t *d_tu_info, uint32_t n_sets,
                                     const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set,
                                     const uint32_t *d_out_set, uint32_t *d_out_state, uint8_t *d_out_rate) {
  if (!sets_args_ok(n_sub, n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  const cabac::CtxSets sets{n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate};
  return write_plan_device_impl(c, n_sub, {d_desc, d_plan, d_values_in, d_tile_first, d_tu, d_tu_at, d_tu_guard}, n_tu, d_coeff, coeff_bytes,
                                {d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info}, d_values_out, &sets, nullptr);
}

// ---- the plan write in pieces (cabac_hip_plan_continue.h): the plan write's two walks over one piece of every substream's plan,
// the encoder in pieces on the expanded records into the caller's slots, the stops.  One wait: the expanded length sizes the
// record scratch.  Not a call of the fixed workspace.
int cabac_hip_plan_continue_write_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint32_t *d_plan,
                                         const uint32_t *d_values_in, const uint32_t *d_tile_first, uint32_t n_tu,
                                         const cabac_tu_desc *d_tu, const uint32_t *d_tu_at, const uint32_t *d_tu_guard,
                                         const void *d_coeff, int coeff_bytes, uint8_t *d_bytes, cabac_substream_result *d_results,
                                         uint32_t *d_values_out, uint32_t *d_tu_info, uint32_t n_sets, const uint32_t *d_state,
                                         const uint8_t *d_rate, const uint32_t *d_start_set, const uint32_t *d_out_set,
                                         uint32_t *d_out_state, uint8_t *d_out_rate, const void *d_coder_in, void *d_coder_out) {
  if (!c || (n_sub && (!d_desc || !d_tile_first || !d_bytes || !d_results)) || (n_tu && (!d_tu || !d_coeff)) ||
      !sets_args_ok(n_sub, n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (coeff_bytes != 4 && coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (n_sub == 0 && n_tu) return fail(c, CABAC_HIP_ERR_INVALID, "blocks without a substream");
  if (c->ws_fixed)
    return fail(c, CABAC_HIP_ERR_INVALID, "the workspace is fixed: the plan write in pieces waits for its sizes; call cabac_hip_workspace_release first");
  if (n_sub == 0) return CABAC_HIP_OK;
  DeviceGuard g(c->device);
  int rc;
  PlanWriteTables w;
  if ((rc = plan_write_tables(c, n_sub, n_tu, true, &w))) return rc;
  uint32_t *out_live = w.words;  // the out sets of the pieces that are coded
  const cabac::PlanWriteIn in{d_desc, d_plan, d_values_in, d_tile_first, d_tu, d_tu_at, d_tu_guard, w.cnt, w.info};
  cabac::CtxPieces pieces{{n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate},
                          static_cast<const cabac_coder_state *>(d_coder_in), static_cast<cabac_coder_state *>(d_coder_out)};
  c->timed = false;
  {  // sizes and info words of ALL blocks of the pieces
    Timed t(c, 5);
    HIP_TRY(c, cabac::launch_residual(c->stream, n_tu, d_tu, d_coeff, coeff_bytes, nullptr, w.cnt, w.info, nullptr, c->d_buf[kResidualScratch]));
  }
  {
    Timed t(c, 28);
    HIP_TRY(c, cabac::launch_plan_resolve_pieces(c->stream, n_sub, in, pieces, w.sub_n, w.sub_cap, w.sub_flag, w.err));
    HIP_TRY(c, cabac::launch_splice_scan(c->stream, n_sub, w.sub_n, w.sub_cap, w.rec_base, w.byte_base, w.err, w.totals, nullptr));
  }
  // (the caller's slots take the bytes: the expanded length decides the record scratch alone)
  if ((rc = wait_for_totals(c, w.totals, "a piece outgrows 32 bits of records", false))) return rc;
  auto *exp_rec = static_cast<uint16_t *>(c->d_buf[kSpRec]);
  {
    Timed t(c, 28);
    HIP_TRY(c, cabac::launch_plan_emit_pieces(c->stream, n_sub, in, w.sub_n, w.sub_flag, w.rec_base, w.desc2, w.tus2, w.tu_off, exp_rec,
                                              d_values_out, d_tu_info));
    if (d_out_set) {  // a piece that is not coded writes no set
      HIP_TRY(c, cabac::launch_plan_out_sets(c->stream, n_sub, w.sub_flag, d_out_set, out_live));
      pieces.out_set = out_live;
    }
  }
  {  // block records of the coded blocks, straight into the expanded pieces
    Timed t(c, 5);
    HIP_TRY(c, cabac::launch_residual(c->stream, n_tu, w.tus2, d_coeff, coeff_bytes, w.tu_off, w.cnt, w.info, exp_rec, c->d_buf[kResidualScratch]));
  }
  {
    Timed t(c, 51);
    HIP_TRY(c, cabac::launch_encode_pieces(c->stream, n_sub, w.desc2, exp_rec, d_bytes, d_results, pieces, piece_encoder_for(c, n_sub)));
    HIP_TRY(c, cabac::launch_plan_stops_pieces(c->stream, n_sub, w.sub_flag, d_results, pieces.coder_out));
  }
  return CABAC_HIP_OK;
}

int cabac_hip_plan_write_rows_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint32_t *d_plan,
                                     const uint32_t *d_values_in, const uint32_t *d_tile_first, uint32_t n_tu, const cabac_tu_desc *d_tu,
                                     const uint32_t *d_tu_at, const uint32_t *d_tu_guard, const void *d_coeff, int coeff_bytes,
                                     uint8_t *d_payload, uint64_t payload_capacity, uint64_t *d_payload_offsets,
                                     cabac_substream_result *d_results, uint32_t *d_values_out, uint32_t *d_tu_info, uint32_t n_level,
                                     const uint32_t *level_first, const uint32_t *d_sync_from, const uint32_t *d_sync_at) {
  const Rows rows{n_level, level_first, d_sync_from, d_sync_at};
  return write_plan_device_impl(c, n_sub, {d_desc, d_plan, d_values_in, d_tile_first, d_tu, d_tu_at, d_tu_guard}, n_tu, d_coeff, coeff_bytes,
                                {d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info}, d_values_out, nullptr, &rows);
}

int cabac_hip_plan_write_rows_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint32_t *plan,
                                    const uint32_t *values_in, uint64_t n_elements_total, const uint32_t *tile_first,
                                    const cabac_tu_desc *tus, const uint32_t *tu_at, const uint32_t *tu_guard, const void *coeff,
                                    int coeff_bytes, uint64_t n_coeff_total, uint8_t *payload, uint64_t payload_capacity,
                                    uint64_t *payload_offsets, cabac_substream_result *results, uint32_t *values_out, uint32_t *tu_info,
                                    uint32_t n_level, const uint32_t *level_first, const uint32_t *sync_from, const uint32_t *sync_at) {
  const Rows rows{n_level, level_first, sync_from, sync_at};
  return host_call_exit(c, write_plan_batch_impl(c, n_sub, desc, plan, values_in, n_elements_total, tile_first, tus, tu_at, tu_guard,
                                                 coeff, coeff_bytes, n_coeff_total, payload, payload_capacity, payload_offsets, results,
                                                 values_out, tu_info, &rows));
}

// ---- spliced rows (cabac_hip_splice_rows.h): the splice pipeline and the winner log's emit from and into sets, and in WPP rows ----
int cabac_hip_encode_residual_sets_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                          const uint32_t *d_splice_first, const cabac_splice *d_splices, uint32_t n_splice, uint32_t n_tu,
                                          const cabac_tu_desc *d_tu, const void *d_coeff, int coeff_bytes, uint8_t *d_payload,
                                          uint64_t payload_capacity, uint64_t *d_payload_offsets, cabac_substream_result *d_results,
                                          uint32_t *d_tu_info, uint32_t *d_bin_counts, uint32_t n_sets, const uint32_t *d_state,
                                          const uint8_t *d_rate, const uint32_t *d_start_set, const uint32_t *d_out_set,
                                          uint32_t *d_out_state, uint8_t *d_out_rate) {
  if (!sets_args_ok(n_sub, n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  const cabac::CtxSets sets{n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate};
  return encode_residual_device_impl(c, n_sub, {d_desc, d_records, d_splice_first, d_splices, n_splice, n_tu, d_tu, d_coeff, coeff_bytes},
                                     {d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info}, d_bin_counts, &sets, nullptr);
}

int cabac_hip_encode_residual_rows_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                          const uint32_t *d_splice_first, const cabac_splice *d_splices, uint32_t n_splice, uint32_t n_tu,
                                          const cabac_tu_desc *d_tu, const void *d_coeff, int coeff_bytes, uint8_t *d_payload,
                                          uint64_t payload_capacity, uint64_t *d_payload_offsets, cabac_substream_result *d_results,
                                          uint32_t *d_tu_info, uint32_t *d_bin_counts, uint32_t n_level, const uint32_t *level_first,
                                          const uint32_t *d_sync_from, const uint32_t *d_sync_at, const uint32_t *d_sync_splice) {
  const Rows rows{n_level, level_first, d_sync_from, d_sync_at, d_sync_splice};
  return encode_residual_device_impl(c, n_sub, {d_desc, d_records, d_splice_first, d_splices, n_splice, n_tu, d_tu, d_coeff, coeff_bytes},
                                     {d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info}, d_bin_counts, nullptr, &rows);
}

int cabac_hip_encode_residual_rows_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                         uint64_t n_records_total, const uint32_t *splice_first, const cabac_splice *splices, uint32_t n_tu,
                                         const cabac_tu_desc *tus, const void *coeff, int coeff_bytes, uint64_t n_coeff_total,
                                         uint8_t *payload, uint64_t payload_capacity, uint64_t *payload_offsets,
                                         cabac_substream_result *results, uint32_t *tu_info, uint32_t *bin_counts, uint32_t n_level,
                                         const uint32_t *level_first, const uint32_t *sync_from, const uint32_t *sync_at,
                                         const uint32_t *sync_splice) {
  const Rows rows{n_level, level_first, sync_from, sync_at, sync_splice};
  return host_call_exit(c, encode_batch_residual_impl(c, n_sub, desc, records, n_records_total, splice_first, splices, n_tu, tus, coeff,
                                                      coeff_bytes, n_coeff_total, payload, payload_capacity, payload_offsets, results,
                                                      tu_info, bin_counts, &rows));
}

int cabac_hip_search_log_mark_device(cabac_search_log *log, uint32_t n, const uint32_t *d_chain) {
  if (!log) return CABAC_HIP_ERR_INVALID;
  cabac_hip_ctx *c = log->ctx;
  if (n && !d_chain) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (n == 0) return CABAC_HIP_OK;
  DeviceGuard g(c->device);
  c->timed = false;
  Timed t(c, 38);
  HIP_TRY(c, cabac::launch_search_log_mark(c->stream, log->a, n, d_chain));
  return CABAC_HIP_OK;
}

int cabac_hip_search_log_encode_sets_device(cabac_search_log *log, const cabac_substream_desc *d_desc, uint8_t *d_payload,
                                            uint64_t payload_capacity, uint64_t *d_payload_offsets, cabac_substream_result *d_results,
                                            uint32_t *d_tu_info, uint32_t *d_bin_counts, uint32_t n_sets, const uint32_t *d_state,
                                            const uint8_t *d_rate, const uint32_t *d_start_set, const uint32_t *d_out_set,
                                            uint32_t *d_out_state, uint8_t *d_out_rate) {
  if (!log) return CABAC_HIP_ERR_INVALID;
  if (!sets_args_ok(log->a.n_chain, n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate))
    return fail(log->ctx, CABAC_HIP_ERR_INVALID, "null");
  const cabac::CtxSets sets{n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate};
  return search_log_encode_impl(log, d_desc, {d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info}, d_bin_counts, &sets,
                                nullptr);
}

int cabac_hip_search_log_encode_rows_device(cabac_search_log *log, const cabac_substream_desc *d_desc, uint8_t *d_payload,
                                            uint64_t payload_capacity, uint64_t *d_payload_offsets, cabac_substream_result *d_results,
                                            uint32_t *d_tu_info, uint32_t *d_bin_counts, uint32_t n_level, const uint32_t *level_first,
                                            const uint32_t *d_sync_from) {
  if (!log) return CABAC_HIP_ERR_INVALID;
  if (!d_sync_from) return fail(log->ctx, CABAC_HIP_ERR_INVALID, "null");
  if (int bad = check_levels(log->ctx, log->a.n_chain, n_level, level_first)) return bad;  // before the first wait
  const Rows rows{n_level, level_first, d_sync_from, nullptr, nullptr};
  return search_log_encode_impl(log, d_desc, {d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info}, d_bin_counts, nullptr,
                                &rows);
}

// ---- sparse coefficient transport (cabac_hip_sparse.h; kernels: cabac_sparse.hip, the CPU forms: cabac_sparse_host.cpp) ----------
namespace {
int sparse_args(cabac_hip_ctx *c, int coeff_bytes, uint64_t n_coeff_total) {
  if (coeff_bytes != 4 && coeff_bytes != 2) return fail(c, CABAC_HIP_ERR_INVALID, "coeff_bytes must be 4 or 2");
  if (n_coeff_total >> 32) return fail(c, CABAC_HIP_ERR_INVALID, "n_coeff_total must be below 2^32 (ent_first is 32-bit)");
  return CABAC_HIP_OK;
}
}  // namespace

int cabac_hip_sparse_expand_device(cabac_hip_ctx *c, uint32_t n_tu, const cabac_tu_desc *d_tu, const uint32_t *d_ent_first,
                                   const uint32_t *d_entries, uint64_t n_entries_max, void *d_coeff, int coeff_bytes,
                                   uint64_t n_coeff_total, cabac_sparse_status *d_status) {
  if (!c || !d_status || !d_ent_first || (n_tu && !d_tu) || (n_entries_max && !d_entries) || (n_coeff_total && !d_coeff))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (int bad = sparse_args(c, coeff_bytes, n_coeff_total)) return bad;
  DeviceGuard g(c->device);
  if (int rc = ensure(c, kSparseScratch, cabac::sparse_scratch_bytes(n_tu))) return rc;
  return TIMED_LAUNCH(c, 41, cabac::launch_sparse_expand(c->stream, n_tu, d_tu, d_ent_first, d_entries, n_entries_max, d_coeff, coeff_bytes,
                                                         n_coeff_total, d_status, c->d_buf[kSparseScratch]));
}

int cabac_hip_sparse_compact_device(cabac_hip_ctx *c, uint32_t n_tu, const cabac_tu_desc *d_tu, const void *d_coeff, int coeff_bytes,
                                    uint64_t n_coeff_total, uint32_t *d_ent_first, uint32_t *d_entries, uint64_t entry_capacity,
                                    cabac_sparse_status *d_status) {
  if (!c || !d_status || !d_ent_first || (n_tu && !d_tu) || (entry_capacity && !d_entries) || (n_coeff_total && !d_coeff))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (int bad = sparse_args(c, coeff_bytes, n_coeff_total)) return bad;
  DeviceGuard g(c->device);
  if (int rc = ensure(c, kSparseScratch, cabac::sparse_scratch_bytes(n_tu))) return rc;
  return TIMED_LAUNCH(c, 42, cabac::launch_sparse_compact(c->stream, n_tu, d_tu, d_coeff, coeff_bytes, n_coeff_total, d_ent_first, d_entries,
                                                          entry_capacity, d_status, c->d_buf[kSparseScratch]));
}

int cabac_hip_sparse_encode_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                  uint64_t n_records_total, const uint32_t *splice_first, const cabac_splice *splices, uint32_t n_tu,
                                  const cabac_tu_desc *tus, const uint32_t *ent_first, const uint32_t *entries, uint64_t n_entries_total,
                                  uint64_t n_coeff_total, uint8_t *payload, uint64_t payload_capacity, uint64_t *payload_offsets,
                                  cabac_substream_result *results, uint32_t *tu_info, uint32_t *bin_counts) {
  if (!c || !ent_first || (n_entries_total && !entries)) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (int bad = sparse_args(c, 2, n_coeff_total)) return bad;
  const SparseSrc sparse{ent_first, entries, n_entries_total};
  return host_call_exit(c, encode_batch_residual_impl(c, n_sub, desc, records, n_records_total, splice_first, splices, n_tu, tus, nullptr, 2,
                                                      n_coeff_total, payload, payload_capacity, payload_offsets, results, tu_info,
                                                      bin_counts, nullptr, &sparse));
}

int cabac_hip_sparse_parse_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *bytes,
                                 uint64_t bytes_total, const uint32_t *tile_first, const cabac_tu_desc *tus, uint32_t *ent_first,
                                 uint32_t *entries, uint64_t entry_capacity, uint64_t n_coeff_total, uint32_t *tu_info,
                                 cabac_substream_result *results, cabac_sparse_status *status) {
  if (!c || !status || !ent_first || (entry_capacity && !entries) || (n_sub && (!desc || !bytes || !tile_first || !tus || !results)))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (int bad = sparse_args(c, 2, n_coeff_total)) return bad;
  if (n_sub == 0) {
    ent_first[0] = 0;
    *status = cabac_sparse_status{0, 0, CABAC_SPARSE_NO_BAD};
    return CABAC_HIP_OK;
  }
  const uint32_t n_tu = tile_first[n_sub];
  for (uint32_t s = 0; s < n_sub; s++)
    if (int bad = check_substream_host(c, desc[s], tile_first, s, &bytes_total)) return bad;
  if (int bad = check_coeff_ranges_host(c, n_tu, tus, n_coeff_total)) return bad;
  const uint64_t cap = std::min(entry_capacity, n_coeff_total);  // blocks that do not overlap hold no more entries than elements
  DeviceGuard g(c->device);
  ParseStage st{c, n_sub, n_tu, 2, n_coeff_total, n_coeff_total != 0};
  int rc;
  if ((rc = st.stage(desc, bytes, bytes_total, tile_first, tus, nullptr, nullptr))) return rc;  // 16-bit blocks: cleared, nothing goes up
  const size_t first_bytes = (size_t(n_tu) + 1) * sizeof(uint32_t);
  Stage own{c};
  auto *d_ent_first = own.room<uint32_t>(kSparseFirst, size_t(n_tu) + 1);
  auto *d_entries = own.room<uint32_t>(kSparseEnt, cap);
  void *d_scratch = own.bytes(kSparseScratch, cabac::sparse_scratch_bytes(n_tu), nullptr, 0);
  auto *d_status = own.room<cabac_sparse_status>(kSparseStatus, 1);
  if (own.rc) return own.rc;
  if ((rc = residual_parse_device_impl(c, n_sub, st.in))) return rc;
  if ((rc = TIMED_LAUNCH(c, 42, cabac::launch_sparse_compact(c->stream, n_tu, st.in.tus, st.in.coeff, 2, n_coeff_total, d_ent_first, d_entries, cap,
                                                             d_status, d_scratch))))
    return rc;
  HIP_TRY(c, down(c, status, d_status, sizeof(cabac_sparse_status)));
  HIP_TRY(c, down(c, ent_first, d_ent_first, first_bytes));
  st.blocks = false;  // the blocks stay on the device: the entries leave in their place, once their number is known
  const int flagged = st.finish(nullptr, tu_info, results);  // the first wait
  if (flagged != CABAC_HIP_OK && flagged != CABAC_HIP_ERR_SUBSTREAM) return flagged;
  if (status->n_entries > entry_capacity)
    return fail(c, CABAC_HIP_ERR_INVALID, "entry_capacity too small (status->n_entries is the size needed)");
  if (status->n_entries > cap) return fail(c, CABAC_HIP_ERR_INVALID, "more entries than coefficients: blocks overlap");
  HIP_TRY(c, down(c, entries, d_entries, status->n_entries * sizeof(uint32_t)));
  HIP_TRY(c, wait_stream(c, c->stream));  // the second
  return flagged;
}

// ---- packed bin records (cabac_hip_rec10.h; kernels: cabac_rec10.hip, the CPU forms: cabac_rec10_host.cpp) ----------------------
namespace {
bool misaligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

// what the three host-pointer forms refuse before they look at anything else
int rec10_host_args(cabac_hip_ctx *c, const uint8_t *packed, uint64_t packed_bytes, uint64_t n_records_total) {
  if (!c || (n_records_total && !packed)) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (n_records_total > UINT64_MAX - 63u || packed_bytes < CABAC_REC10_BYTES(n_records_total))
    return fail(c, CABAC_HIP_ERR_INVALID, "packed_bytes below CABAC_REC10_BYTES(n_records_total)");
  return CABAC_HIP_OK;
}
}  // namespace

int cabac_hip_rec10_unpack_device(cabac_hip_ctx *c, const uint8_t *d_packed, uint64_t first, uint64_t n, uint16_t *d_records) {
  if (!c || (n && (!d_packed || !d_records))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (misaligned16(d_packed)) return fail(c, CABAC_HIP_ERR_INVALID, "d_packed must be 16-byte aligned");
  if (first > UINT64_MAX - 7u || n > UINT64_MAX - 7u - first) return fail(c, CABAC_HIP_ERR_INVALID, "first + n out of range");
  DeviceGuard g(c->device);
  return TIMED_LAUNCH(c, 43, cabac::launch_rec10_unpack(c->stream, d_packed, first, n, d_records));
}

int cabac_hip_rec10_pack_device(cabac_hip_ctx *c, const uint16_t *d_records, uint64_t n_records, uint8_t *d_packed,
                                uint64_t packed_capacity, cabac_rec10_status *d_status) {
  if (!c || !d_status || (n_records && (!d_records || !d_packed))) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (misaligned16(d_packed)) return fail(c, CABAC_HIP_ERR_INVALID, "d_packed must be 16-byte aligned");
  if (n_records > UINT64_MAX - 63u) return fail(c, CABAC_HIP_ERR_INVALID, "n_records out of range");
  DeviceGuard g(c->device);
  return TIMED_LAUNCH(c, 44, cabac::launch_rec10_pack(c->stream, d_records, n_records, d_packed, packed_capacity, d_status));
}

int cabac_hip_rec10_encode_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *packed,
                                 uint64_t packed_bytes, uint64_t n_records_total, uint8_t *bytes, uint64_t bytes_total,
                                 cabac_substream_result *results) {
  if (int bad = rec10_host_args(c, packed, packed_bytes, n_records_total)) return bad;
  return host_call_exit(c, encode_batch_impl(c, n_sub, desc, packed, n_records_total, bytes, bytes_total, nullptr, 0, nullptr, results, true));
}

int cabac_hip_rec10_encode_batch_payload(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *packed,
                                         uint64_t packed_bytes, uint64_t n_records_total, uint8_t *payload, uint64_t payload_capacity,
                                         uint64_t *payload_offsets, cabac_substream_result *results) {
  if (!payload || !payload_offsets) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (int bad = rec10_host_args(c, packed, packed_bytes, n_records_total)) return bad;
  uint64_t slots_end = 0;  // as in cabac_hip_encode_batch_payload
  for (uint32_t s = 0; s < n_sub && desc; s++) slots_end = std::max<uint64_t>(slots_end, desc[s].byte_offset + desc[s].byte_capacity);
  return host_call_exit(c, encode_batch_impl(c, n_sub, desc, packed, n_records_total, nullptr, slots_end, payload, payload_capacity,
                                             payload_offsets, results, true));
}

int cabac_hip_rec10_decode_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint8_t *packed,
                                 uint64_t packed_bytes, uint64_t n_records_total, const uint8_t *bytes, uint64_t bytes_total,
                                 uint8_t *bins, int bins_packed, cabac_substream_result *results) {
  if (int bad = rec10_host_args(c, packed, packed_bytes, n_records_total)) return bad;
  return host_call_exit(c, decode_batch_impl(c, n_sub, desc, packed, n_records_total, bytes, bytes_total, bins, results, bins_packed != 0,
                                             true));
}

// ---- the fixed workspace (cabac_hip_workspace.h; the gate and its kernels: cabac_workspace.hip) -------------------------------
int cabac_hip_workspace_bound(uint32_t n_sub, uint64_t n_host_records, uint32_t n_tu, uint64_t n_coded_coeff, uint64_t *expanded_records,
                              uint64_t *slot_bytes) {
  if (!expanded_records || !slot_bytes) return CABAC_HIP_ERR_INVALID;
  const uint64_t lim = uint64_t(1) << 60;
  if (n_host_records > lim / 64 || n_coded_coeff > lim / 64) return CABAC_HIP_ERR_INVALID;
  // the sum of CABAC_TU_MAX_RECORDS(n) = 33 + 38 n over the blocks; a slot: slot_bytes() of cabac_splice.hip, < 7 n / 8 + 24
  const uint64_t rec = n_host_records + 33u * uint64_t(n_tu) + 38u * n_coded_coeff;
  *expanded_records = rec;
  *slot_bytes = (7u * rec + 7u) / 8u + 24u * uint64_t(n_sub);
  return CABAC_HIP_OK;
}

int cabac_hip_workspace_fix(cabac_hip_ctx *c, const cabac_workspace_sizes *sizes) {
  if (!c || !sizes) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  const cabac_workspace_sizes z = *sizes;
  const uint64_t lim = uint64_t(1) << 60;
  if (z.reserved != 0 || (z.flags & ~CABAC_WS_ROWS) != 0) return fail(c, CABAC_HIP_ERR_INVALID, "reserved or unknown flags");
  if (z.n_entries > lim || z.expanded_records > lim || z.slot_bytes > lim || z.log_records > lim)
    return fail(c, CABAC_HIP_ERR_INVALID, "a size beyond 2^60");
  DeviceGuard g(c->device);
  HIP_TRY(c, wait_stream(c, c->stream));  // what is queued may use the buffers that grow below
  c->ws_fixed = false;
  const size_t n_s = z.n_sub ? z.n_sub : 1, n_blk = z.n_tu ? z.n_tu : 1;
  const size_t n_pre = size_t(z.n_tu) + z.n_sub + 1;
  const size_t plan32 = ((n_pre + 2 * size_t(z.n_sub) + n_blk + 2) + 1) & ~size_t(1);  // encode_residual_device_impl's kSpPlan
  const size_t pw32 = (3 * n_s + 2 + 1) & ~size_t(1);                                   // write_plan_device_impl's kPwPlan
  const struct {
    int slot;
    size_t bytes;
  } need[] = {
      {kRowsWords, 2 * n_s * sizeof(uint32_t)},
      {kSpCnt, 2 * n_blk * sizeof(uint32_t)},
      {kResidualScratch, cabac::residual_scratch_bytes(z.n_tu)},
      {kSpPlan, plan32 * sizeof(uint32_t) + (2 * size_t(z.n_sub) + 3) * sizeof(uint64_t)},
      {kSpDesc, n_s * sizeof(cabac_substream_desc)},
      {kSpTuOff, n_blk * sizeof(uint64_t)},
      {kSpFlag, 64},
      {kSpRec, (z.expanded_records + 64) * sizeof(uint16_t)},
      {kSpBytes, z.slot_bytes + 64},
      {kPwPlan, pw32 * sizeof(uint32_t) + (2 * n_s + 3) * sizeof(uint64_t)},
      {kPwTu, n_blk * sizeof(cabac_tu_desc)},
      {kLogDesc, n_s * sizeof(cabac_substream_desc)},
      {kLogFirst, (n_s + 1) * sizeof(uint32_t)},
      {kLogRec, (z.log_records + 8) * sizeof(uint16_t)},
      {kLogSplice, n_blk * sizeof(cabac_splice)},
  };
  for (const auto &n : need)
    if (int rc = ensure(c, n.slot, n.bytes)) return rc;
  if (z.flags & CABAC_WS_ROWS) {  // wpp_device_impl's slots
    const size_t set_words = n_s * CABAC_NUM_CONTEXTS;
    int rc;
    if ((rc = ensure(c, kWppState, set_words * sizeof(uint32_t))) || (rc = ensure(c, kWppRate, set_words)) ||
        (rc = ensure(c, kWppDesc, n_s * sizeof(cabac_substream_desc))) || (rc = ensure(c, kWppIndex, 2 * n_s * sizeof(uint32_t))))
      return rc;
  }
  if (!c->h_totals) HIP_TRY(c, pinned_alloc(c, &c->h_totals, 64, hipHostMallocDefault));
  if (!c->d_ws && device_alloc(c, &c->d_ws, sizeof(cabac::WsState)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, CABAC_HIP_ERR_NOMEM, "hipMalloc failed");
  }
  cabac::WsState init = {};
  init.status.first_voided = CABAC_WS_NONE_VOIDED;
  init.rec_cap = z.expanded_records;
  init.slot_cap = z.slot_bytes;
  HIP_TRY(c, hipMemcpyAsync(c->d_ws, &init, sizeof init, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, wait_stream(c, c->stream));  // `init` leaves scope
  c->ws = z;
  c->ws_fixed = true;
  return CABAC_HIP_OK;
}

namespace {
// the status as it stands when the stream has drained (into *out)
int read_status(cabac_hip_ctx *c, cabac_workspace_status *out) {
  static_assert(sizeof(cabac_workspace_status) <= 64, "the pinned block of the ctx holds the status");
  HIP_TRY(c, hipMemcpyAsync(c->h_totals, &c->d_ws->status, sizeof *out, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, wait_stream(c, c->stream));
  memcpy(out, c->h_totals, sizeof *out);
  return CABAC_HIP_OK;
}
}  // namespace

int cabac_hip_workspace_release(cabac_hip_ctx *c) {
  if (!c) return CABAC_HIP_ERR_INVALID;
  if (!c->ws_fixed) return CABAC_HIP_OK;
  DeviceGuard g(c->device);
  if (int rc = read_status(c, &c->ws_last)) return rc;
  c->ws_fixed = false;
  return CABAC_HIP_OK;
}

int cabac_hip_workspace_status_device(cabac_hip_ctx *c, cabac_workspace_status *d_out) {
  if (!c || !d_out) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (!c->ws_fixed) return fail(c, CABAC_HIP_ERR_INVALID, "the workspace is not fixed");
  DeviceGuard g(c->device);
  HIP_TRY(c, hipMemcpyAsync(d_out, &c->d_ws->status, sizeof *d_out, hipMemcpyDefault, c->stream));
  return CABAC_HIP_OK;
}

int cabac_hip_workspace_status(cabac_hip_ctx *c, cabac_workspace_status *out) {
  if (!c || !out) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (!c->ws_fixed) {
    *out = c->ws_last;
    return CABAC_HIP_OK;
  }
  DeviceGuard g(c->device);
  return read_status(c, out);
}

int cabac_hip_workspace_waits(cabac_hip_ctx *c, uint64_t *n) {
  if (!c || !n) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  *n = c->n_waits;
  return CABAC_HIP_OK;
}

// ---- probe points (cabac_probe.hip, the estimator's probe instantiation; declared in cabac_hip_probe.h) ----------------------
namespace {
bool probe_args_ok(uint32_t n_sub, const void *d_desc, const void *d_records, const uint32_t *d_probe_first, const uint32_t *d_probe_at,
                   uint32_t n_probe, uint32_t n_sets, const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set,
                   const void *d_out) {
  if (n_sub == 0) return true;
  if (!d_desc || !d_records || !d_probe_first || (n_probe && (!d_probe_at || !d_out))) return false;
  return sets_args_ok(n_sub, n_sets, d_state, d_rate, d_start_set, nullptr, nullptr, nullptr);
}

// the two host-pointer forms: one staging, the walk chosen by `estimate` (out: uint64_t[n_probe] then, else uint32_t[n_probe])
int probes_batch_impl(cabac_hip_ctx *c, bool estimate, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                      uint64_t n_records_total, const uint32_t *probe_first, const uint32_t *probe_at, uint32_t n_probe, uint32_t n_sets,
                      const uint32_t *state, const uint8_t *rate, const uint32_t *start_set, void *out, uint32_t *flags) {
  if (!c || (n_sub && (!desc || (n_records_total && !records))) || (n_sub && n_probe && !out)) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  if (n_sub == 0) return CABAC_HIP_OK;
  if (start_set && n_sets && (!state || !rate)) return fail(c, CABAC_HIP_ERR_INVALID, "null");
  for (uint32_t s = 0; s < n_sub; s++) {
    if (int bad = check_records_host(c, s, desc[s], n_records_total)) return bad;
    if (start_set && start_set[s] != CABAC_CTX_NO_SET && start_set[s] >= n_sets) {
      char buf[96];
      snprintf(buf, sizeof buf, "substream %u: start set >= n_sets", s);
      return fail(c, CABAC_HIP_ERR_INVALID, buf);
    }
  }
  if (int bad = check_probes_host(c, n_sub, probe_first, probe_at, n_probe)) return bad;
  DeviceGuard g(c->device);
  int rc;
  const size_t set_entries = size_t(n_sets) * CABAC_NUM_CONTEXTS, each = estimate ? sizeof(uint64_t) : sizeof(uint32_t);
  Stage st{c};
  auto *d_desc = st.put(kDesc, n_sub, desc);
  auto *d_rec = st.put(kRecords, n_records_total, records);
  auto *d_first = st.put(kProbeFirst, size_t(n_sub) + 1, probe_first);
  auto *d_at = st.put(kProbeAt, n_probe, probe_at);
  const uint32_t *d_state = nullptr, *d_set = nullptr;
  const uint8_t *d_rate = nullptr;
  if (start_set) {
    d_state = st.put(kEstInState, set_entries, state);
    d_rate = st.put(kEstInRate, set_entries, rate);
    d_set = st.put(kEstInSet, n_sub, start_set);
  }
  auto *d_flags = st.room<uint32_t>(kFlags, n_sub);
  void *d_out = st.bytes(kProbeOut, size_t(n_probe) * each, nullptr, 0);
  if (st.rc) return st.rc;
  if (estimate)
    rc = cabac_hip_estimate_probes_device(c, n_sub, d_desc, d_rec, d_first, d_at, n_probe, n_sets, d_state, d_rate, d_set,
                                          static_cast<uint64_t *>(d_out), d_flags);
  else
    rc = cabac_hip_written_bits_device(c, n_sub, d_desc, d_rec, d_first, d_at, n_probe, n_sets, d_state, d_rate, d_set,
                                       static_cast<uint32_t *>(d_out), d_flags);
  if (rc) return rc;
  // the values come back into the ctx's own memory first: a caller's array holds only what the list's probes own
  std::vector<uint32_t> fl(n_sub);
  std::vector<uint8_t> vals(size_t(n_probe) * each);
  HIP_TRY(c, down(c, vals.data(), d_out, vals.size()));
  HIP_TRY(c, down(c, fl.data(), d_flags, n_sub * sizeof(uint32_t)));
  HIP_TRY(c, wait_stream(c, c->stream));
  std::memcpy(out, vals.data(), size_t(probe_first[n_sub]) * each);
  return flags_status(c, n_sub, fl.data(), flags, "substream flag set (see flags[])");
}
}  // namespace

int cabac_hip_written_bits_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                  const uint32_t *d_probe_first, const uint32_t *d_probe_at, uint32_t n_probe, uint32_t n_sets,
                                  const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set, uint32_t *d_bits,
                                  uint32_t *d_flags) {
  if (!c || !probe_args_ok(n_sub, d_desc, d_records, d_probe_first, d_probe_at, n_probe, n_sets, d_state, d_rate, d_start_set, d_bits))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  return TIMED_LAUNCH(c, 45, cabac::launch_written_bits(c->stream, n_sub, d_desc, d_records, cabac::ProbeList{d_probe_first, d_probe_at, n_sets},
                                                         d_state, d_rate, d_start_set, d_bits, d_flags));
}

int cabac_hip_estimate_probes_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                     const uint32_t *d_probe_first, const uint32_t *d_probe_at, uint32_t n_probe, uint32_t n_sets,
                                     const uint32_t *d_state, const uint8_t *d_rate, const uint32_t *d_start_set, uint64_t *d_frac_bits,
                                     uint32_t *d_flags) {
  if (!c || !probe_args_ok(n_sub, d_desc, d_records, d_probe_first, d_probe_at, n_probe, n_sets, d_state, d_rate, d_start_set, d_frac_bits))
    return fail(c, CABAC_HIP_ERR_INVALID, "null");
  DeviceGuard g(c->device);
  return TIMED_LAUNCH(c, 46, cabac::launch_estimate_probes(c->stream, n_sub, d_desc, d_records,
                                                            cabac::ProbeList{d_probe_first, d_probe_at, n_sets}, d_state, d_rate, d_start_set,
                                                            d_frac_bits, d_flags));
}

int cabac_hip_written_bits_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                 uint64_t n_records_total, const uint32_t *probe_first, const uint32_t *probe_at, uint32_t n_probe,
                                 uint32_t n_sets, const uint32_t *state, const uint8_t *rate, const uint32_t *start_set, uint32_t *bits,
                                 uint32_t *flags) {
  return probes_batch_impl(c, false, n_sub, desc, records, n_records_total, probe_first, probe_at, n_probe, n_sets, state, rate, start_set,
                           bits, flags);
}

int cabac_hip_estimate_probes_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                    uint64_t n_records_total, const uint32_t *probe_first, const uint32_t *probe_at, uint32_t n_probe,
                                    uint32_t n_sets, const uint32_t *state, const uint8_t *rate, const uint32_t *start_set,
                                    uint64_t *frac_bits, uint32_t *flags) {
  return probes_batch_impl(c, true, n_sub, desc, records, n_records_total, probe_first, probe_at, n_probe, n_sets, state, rate, start_set,
                           frac_bits, flags);
}

int cabac_hip_encode_residual_probes_device(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *d_desc, const uint16_t *d_records,
                                            const uint32_t *d_splice_first, const cabac_splice *d_splices, uint32_t n_splice, uint32_t n_tu,
                                            const cabac_tu_desc *d_tu, const void *d_coeff, int coeff_bytes, uint8_t *d_payload,
                                            uint64_t payload_capacity, uint64_t *d_payload_offsets, cabac_substream_result *d_results,
                                            uint32_t *d_tu_info, uint32_t *d_bin_counts, const uint32_t *d_probe_first,
                                            const uint32_t *d_probe_at, const uint32_t *d_probe_splice, uint32_t n_probe, uint32_t *d_bits) {
  const SpliceProbes probes{d_probe_first, d_probe_at, d_probe_splice, n_probe, d_bits};
  return encode_residual_device_impl(c, n_sub, {d_desc, d_records, d_splice_first, d_splices, n_splice, n_tu, d_tu, d_coeff, coeff_bytes},
                                     {d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info}, d_bin_counts, nullptr, nullptr,
                                     nullptr, &probes);
}

int cabac_hip_encode_residual_probes_batch(cabac_hip_ctx *c, uint32_t n_sub, const cabac_substream_desc *desc, const uint16_t *records,
                                           uint64_t n_records_total, const uint32_t *splice_first, const cabac_splice *splices,
                                           uint32_t n_tu, const cabac_tu_desc *tus, const void *coeff, int coeff_bytes,
                                           uint64_t n_coeff_total, uint8_t *payload, uint64_t payload_capacity, uint64_t *payload_offsets,
                                           cabac_substream_result *results, uint32_t *tu_info, uint32_t *bin_counts,
                                           const uint32_t *probe_first, const uint32_t *probe_at, const uint32_t *probe_splice,
                                           uint32_t n_probe, uint32_t *bits) {
  const SpliceProbes probes{probe_first, probe_at, probe_splice, n_probe, bits};
  return host_call_exit(c, encode_batch_residual_impl(c, n_sub, desc, records, n_records_total, splice_first, splices, n_tu, tus, coeff,
                                                      coeff_bytes, n_coeff_total, payload, payload_capacity, payload_offsets, results,
                                                      tu_info, bin_counts, nullptr, nullptr, &probes));
}

int cabac_hip_host_alloc(size_t bytes, void **out) {
  if (!out) return CABAC_HIP_ERR_INVALID;
  *out = nullptr;
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return CABAC_HIP_ERR_NOMEM;
  }
  std::lock_guard<std::mutex> lk(g_host_mu);
  g_host_owned[p] = bytes ? bytes : 16;
  *out = p;
  return CABAC_HIP_OK;
}

int cabac_hip_host_free(void *p) {
  if (!p) return CABAC_HIP_OK;
  {
    std::lock_guard<std::mutex> lk(g_host_mu);
    if (!g_host_owned.erase(p)) return CABAC_HIP_ERR_INVALID;
  }
  return hipHostFree(p) == hipSuccess ? CABAC_HIP_OK : CABAC_HIP_ERR_HIP;
}

int cabac_hip_host_register(void *p, size_t bytes) {
  if (!p || !bytes) return CABAC_HIP_ERR_INVALID;
  if (hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) {
    (void)hipGetLastError();
    return CABAC_HIP_ERR_HIP;
  }
  std::lock_guard<std::mutex> lk(g_host_mu);
  g_host_registered[p] = bytes;
  return CABAC_HIP_OK;
}

int cabac_hip_host_unregister(void *p) {
  {
    std::lock_guard<std::mutex> lk(g_host_mu);
    if (!g_host_registered.erase(p)) return CABAC_HIP_ERR_INVALID;
  }
  return hipHostUnregister(p) == hipSuccess ? CABAC_HIP_OK : CABAC_HIP_ERR_HIP;
}

int cabac_hip_host_is_pinned(const void *p, size_t bytes) { return host_is_pinned(p, bytes) ? 1 : 0; }

#ifdef CABAC_PARSE_PROFILE
int cabac_hip_debug_parse_waves(unsigned long long *out) { return cabac::debug_read_parse_waves(out) == hipSuccess ? 0 : -3; }
int cabac_hip_debug_parse_prof(unsigned long long *out) { return cabac::debug_read_parse_prof(out) == hipSuccess ? 0 : -3; }
#endif

}  // extern "C"
