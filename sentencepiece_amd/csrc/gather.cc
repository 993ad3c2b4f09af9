// spmx_all_gather_ids and the spmx_rccl_* helpers (include/spmx.h): the token ids of every rank on every rank, over
// RCCL, from a C / C++ host -- what BASELINE.json's north_star names ("shards the input corpus across the 8 GPUs of one
// node with a RCCL all-gatherv of the token-id output over xGMI"; the per-sentence semantics are the Python wrapper's
// batch form, python/src/sentencepiece/sentencepiece.i:245-267: the job's sentences in order, each with its own ids).
//
// One process per GPU.  librccl is NOT a link-time dependency of libspmx.so: its entry points are looked up at the
// first call (dlopen of SPMX_RCCL_LIB or "librccl.so"), so single-GPU users never load it.  The gather is
//
//   counts   ncclAllGather of {sentences, ids} of every rank (two uint64 per rank, through device memory), read back;
//   payload  one ncclGroup of exact-size point-to-point transfers: to every peer my ids and my per-sentence offsets,
//            from every peer theirs, straight into their places in the gathered CSR -- xGMI is point to point, so
//            world - 1 concurrent sends per rank is the pattern the links are built for, and nothing is padded to the
//            largest rank (the all-gather of equal-sized blocks sentencepiece_amd/sharding.py also offers is);
//   rebase   one small launch moves every rank's offsets from "ids before me on my rank" to "in the whole job".
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/spmx.h"
#include "launch.h"

using namespace spmx;

namespace {

// the part of rccl.h this file needs (ncclResult_t 0 = ncclSuccess; ncclDataType_t numbers: rccl.h:459-470)
struct NcclUniqueId { char internal[128]; };
enum { kNcclInt8 = 0, kNcclInt32 = 2, kNcclUint64 = 5 };
struct RcclApi {
  int (*GetUniqueId)(NcclUniqueId *) = nullptr;
  int (*CommInitRank)(void **, int, NcclUniqueId, int) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
  int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
  std::string error;
  bool ok = false;
};

RcclApi &Rccl() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    const char *path = getenv("SPMX_RCCL_LIB");
    void *lib = dlopen(path && *path ? path : "librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib && !(path && *path)) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) { api.error = std::string("RCCL is not loadable: ") + dlerror(); return; }
    auto sym = [&](const char *name) -> void * {
      void *p = dlsym(lib, name);
      if (!p && api.error.empty()) api.error = std::string("RCCL lacks ") + name;
      return p;
    };
    api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(sym("ncclGetUniqueId"));
    api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(sym("ncclCommInitRank"));
    api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
    api.AllGather = reinterpret_cast<decltype(api.AllGather)>(sym("ncclAllGather"));
    api.Send = reinterpret_cast<decltype(api.Send)>(sym("ncclSend"));
    api.Recv = reinterpret_cast<decltype(api.Recv)>(sym("ncclRecv"));
    api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(sym("ncclGroupStart"));
    api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(sym("ncclGroupEnd"));
    api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
    api.ok = api.error.empty();
  });
  return api;
}

thread_local std::string t_gather_error;

int FailG(int code, const std::string &msg) {
  t_gather_error = msg;
  return code;
}

#define RCCL_OR_RETURN(api, expr)                                                                              \
  do {                                                                                                         \
    const int r_ = (expr);                                                                                     \
    if (r_ != 0) return FailG(13, std::string(#expr) + ": " + ((api).GetErrorString ? (api).GetErrorString(r_) : "RCCL error")); \
  } while (0)
#define HIPG_OR_RETURN(expr)                                                                 \
  do {                                                                                       \
    const hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) return FailG(13, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

}  // namespace

#ifdef SPMX_EMULATED
// The CPU model of the wavefront (tests/emu) has no kernels.hip: the two launchers of the packed gather run their device
// bodies over the grid there, one workgroup of one wavefront after another.
namespace spmx {
hipError_t LaunchPackIds(const PackArgs &a, int grid, hipStream_t) {
  for (int b = 0; b < grid; ++b) emu::RunWave(b, grid, nullptr, [&] { pack_block(a); });
  return hipSuccess;
}
hipError_t LaunchUnpackIds(const UnpackArgs &a, int grid, hipStream_t) {
  for (int b = 0; b < grid; ++b) emu::RunWave(b, grid, nullptr, [&] { unpack_block(a); });
  return hipSuccess;
}
}  // namespace spmx
constexpr uint64_t kPackedMaxGrid = 3;
#else
constexpr uint64_t kPackedMaxGrid = 8192;    // workgroups of one wavefront: 32 per CU of an MI355X in flight
#endif

namespace {

// workgroups for a streaming pass over `sentences` (a tile each) and `ids` (64 units each)
int PackedGrid(uint64_t sentences, uint64_t ids) {
  const uint64_t t = (sentences + kPackedTile - 1) / kPackedTile, g = (ids + 64 * kPackedUnit - 1) / (64 * kPackedUnit);
  const uint64_t m = t > g ? t : g;
  return static_cast<int>(m < 1 ? 1 : (m > kPackedMaxGrid ? kPackedMaxGrid : m));
}

int PackInto(const PackedLayout &lay, const int32_t *d_ids, const uint64_t *d_id_offsets, uint64_t n, uint64_t out_cap_ids,
             uint64_t out_cap_offs, uint8_t *d_block, hipStream_t stream) {
  PackArgs pa{};
  pa.ids = d_ids;
  pa.offs = d_id_offsets;
  pa.n = n;
  pa.block = d_block;
  pa.lay = lay;
  pa.out_cap_ids = out_cap_ids;
  pa.out_cap_offs = out_cap_offs;
  pa.bad_args = n && !d_id_offsets ? 1u : 0u;
  HIPG_OR_RETURN(hipMemsetAsync(d_block, 0, kPhWords * 8, stream));     // (the status word: the kernel only ORs into it)
  HIPG_OR_RETURN(LaunchPackIds(pa, PackedGrid(n < lay.cap_s ? n : lay.cap_s, lay.cap_i), stream));
  return 0;
}

int UnpackFrom(const PackedLayout &lay, const uint8_t *d_blocks, int world, int32_t *d_all_ids, uint64_t all_ids_capacity,
               uint64_t *d_all_id_offsets, uint64_t all_offsets_capacity, uint64_t *d_rank_sentences, uint64_t *d_rank_ids,
               uint64_t *d_status, hipStream_t stream) {
  UnpackArgs ua{};
  ua.blocks = d_blocks;
  ua.block_stride = lay.bytes;
  ua.world = static_cast<uint32_t>(world);
  ua.lay = lay;
  ua.all_ids = d_all_ids;
  ua.all_offs = d_all_id_offsets;
  ua.cap_ids = all_ids_capacity;
  ua.cap_offs = all_offsets_capacity;
  ua.rank_sentences = d_rank_sentences;
  ua.rank_ids = d_rank_ids;
  ua.status = d_status;
  const uint64_t w = static_cast<uint64_t>(world);
  HIPG_OR_RETURN(LaunchUnpackIds(ua, PackedGrid(lay.cap_s * w, lay.cap_i * w), stream));
  return 0;
}

std::string PackedMessage(const uint64_t st[4]) {
  const uint32_t bits = static_cast<uint32_t>(st[2]);
  const std::string who = st[1] == 0xFFFFFFFFu ? std::string("this caller") : "rank " + std::to_string(st[1]);
  std::string what;
  if (bits & kPsFormat) what = "'s block is not a packed block of this version and these capacities";
  else if (bits & kPsArgs) what = " passed a null id / offset buffer with a non-zero size";
  else if (bits & kPsSentences) what = " has more sentences than the agreed capacity";
  else if (bits & kPsIds) what = " has more ids than the agreed capacity";
  else if (bits & kPsOutput) what = "'s output buffers are too small for the gathered CSR (" + std::to_string(st[3]) + " ids)";
  else if (bits & kPsCount) what = " has a sentence with more ids than the agreed count width holds";
  else if (bits & kPsId) what = " has an id outside the agreed id width";
  return who + what + " (every rank sees this: nothing was written)";
}

}  // namespace

struct spmx_gather_plan {
  void *comm = nullptr;
  int rank = 0, world = 1;
  PackedLayout lay{};
  uint8_t *d_blocks = nullptr;     // world blocks; [rank] is the one this rank packs into and sends from
  uint64_t *d_status = nullptr;    // what the last unpack found (UnpackArgs::status)
  uint64_t *h_status = nullptr;    // pinned: where spmx_gather_plan_status reads it
};

constexpr int kGatherWords = 5;      // per rank in the counts all-gather: sentences, ids, id capacity, offset capacity, arguments valid

extern "C" {

const char *spmx_gather_last_error(void) { return t_gather_error.c_str(); }

int spmx_rccl_unique_id(void *id128) {
  RcclApi &api = Rccl();
  if (!api.ok) return FailG(14, api.error);
  if (!id128) return FailG(3, "null id buffer");
  NcclUniqueId id;
  RCCL_OR_RETURN(api, api.GetUniqueId(&id));
  memcpy(id128, &id, sizeof(id));
  return 0;
}

int spmx_rccl_comm_init(void **comm, int world, int rank, const void *id128) {
  RcclApi &api = Rccl();
  if (!api.ok) return FailG(14, api.error);
  if (!comm || !id128 || world < 1 || rank < 0 || rank >= world) return FailG(3, "bad communicator arguments");
  NcclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  RCCL_OR_RETURN(api, api.CommInitRank(comm, world, id, rank));
  return 0;
}

int spmx_rccl_comm_destroy(void *comm) {
  RcclApi &api = Rccl();
  if (!api.ok) return FailG(14, api.error);
  if (comm) RCCL_OR_RETURN(api, api.CommDestroy(comm));
  return 0;
}

uint64_t spmx_gather_scratch_words(int world) {
  return world >= 1 && world <= kMaxRanks ? static_cast<uint64_t>(kGatherWords) * (1u + static_cast<uint64_t>(world)) : 0u;
}

int spmx_all_gather_ids(void *nccl_comm, int rank, int world, const int32_t *d_ids, uint64_t n_ids,
                        const uint64_t *d_id_offsets, uint64_t n_sentences, int32_t *d_all_ids, uint64_t all_ids_capacity,
                        uint64_t *d_all_id_offsets, uint64_t all_offsets_capacity, uint64_t *d_scratch,
                        uint64_t *rank_sentences, uint64_t *rank_ids, void *stream_) {
  RcclApi &api = Rccl();
  if (!api.ok) return FailG(14, api.error);
  if (world < 1 || world > kMaxRanks || rank < 0 || rank >= world) return FailG(3, "world must be 1 .. 64 and rank inside it");
  if (!nccl_comm || !d_scratch) return FailG(3, "null communicator or scratch");   // (the only errors decided by one rank alone)
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  // ---- counts: {sentences, ids} of every rank -- and what its output buffers hold: whether the gathered CSR fits is
  // decided by ALL ranks from the same numbers, so that either every rank goes on to the transfers or none does (a rank
  // that returned early on a capacity only it knew to be too small would leave its peers waiting in ncclSend / ncclRecv) ----
  const bool args_ok = !(n_sentences && !d_id_offsets) && !(n_ids && !d_ids);
  const uint64_t mine[kGatherWords] = {n_sentences, n_ids, d_all_ids ? all_ids_capacity : 0, d_all_id_offsets ? all_offsets_capacity : 0,
                                       args_ok ? 1u : 0u};
  uint64_t *d_mine = d_scratch, *d_all = d_scratch + kGatherWords;     // scratch: kGatherWords * (1 + world) uint64
  HIPG_OR_RETURN(hipMemcpyAsync(d_mine, mine, sizeof(mine), hipMemcpyHostToDevice, stream));
  RCCL_OR_RETURN(api, api.AllGather(d_mine, d_all, kGatherWords, kNcclUint64, nccl_comm, stream));
  uint64_t got[kGatherWords * kMaxRanks];
  HIPG_OR_RETURN(hipMemcpyAsync(got, d_all, sizeof(uint64_t) * kGatherWords * static_cast<size_t>(world), hipMemcpyDeviceToHost, stream));
  HIPG_OR_RETURN(hipStreamSynchronize(stream));
  uint64_t all[2 * kMaxRanks];
  RebaseArgs ra{};
  ra.world = static_cast<uint32_t>(world);
  for (int r = 0; r < world; ++r) {
    all[2 * r] = got[kGatherWords * r];
    all[2 * r + 1] = got[kGatherWords * r + 1];
    ra.sent_before[r + 1] = ra.sent_before[r] + all[2 * r];
    ra.ids_before[r + 1] = ra.ids_before[r] + all[2 * r + 1];
  }
  if (rank_sentences) memcpy(rank_sentences, ra.sent_before, sizeof(uint64_t) * static_cast<size_t>(world + 1));
  if (rank_ids) memcpy(rank_ids, ra.ids_before, sizeof(uint64_t) * static_cast<size_t>(world + 1));
  const uint64_t total_s = ra.sent_before[world], total_i = ra.ids_before[world];
  for (int r = 0; r < world; ++r)
    if (!got[kGatherWords * r + 4])
      return FailG(3, "rank " + std::to_string(r) + " passed a null id / offset buffer with a non-zero size: no rank transfers anything");
  for (int r = 0; r < world; ++r) {
    const uint64_t cap_i = got[kGatherWords * r + 2], cap_o = got[kGatherWords * r + 3];
    if (total_i > cap_i || total_s + 1 > cap_o)
      return FailG(8, "the gathered CSR needs " + std::to_string(total_i) + " ids and " + std::to_string(total_s + 1) + " offsets; rank " +
                          std::to_string(r) + "'s buffers hold " + std::to_string(cap_i) + " / " + std::to_string(cap_o) +
                          " (every rank returns this: no rank transfers anything)");
  }
  // ---- payload: exact sizes, point to point, one group ----
  RCCL_OR_RETURN(api, api.GroupStart());
  int in_group = 0;                       // (a call that fails inside the group must not leave it open: the first failure is kept, the group closed)
  for (int k = 1; k < world && in_group == 0; ++k) {
    const int to = (rank + k) % world, from = (rank - k + world) % world;    // (every rank a different peer per step)
    if (n_ids && in_group == 0) in_group = api.Send(d_ids, n_ids, kNcclInt32, to, nccl_comm, stream);
    if (n_sentences && in_group == 0) in_group = api.Send(d_id_offsets, n_sentences, kNcclUint64, to, nccl_comm, stream);
    if (all[2 * from + 1] && in_group == 0) in_group = api.Recv(d_all_ids + ra.ids_before[from], all[2 * from + 1], kNcclInt32, from, nccl_comm, stream);
    if (all[2 * from] && in_group == 0) in_group = api.Recv(d_all_id_offsets + ra.sent_before[from], all[2 * from], kNcclUint64, from, nccl_comm, stream);
  }
  const int ended = api.GroupEnd();
  if (in_group != 0) return FailG(13, std::string("ncclSend / ncclRecv: ") + (api.GetErrorString ? api.GetErrorString(in_group) : "RCCL error"));
  RCCL_OR_RETURN(api, ended);
  if (n_ids) HIPG_OR_RETURN(hipMemcpyAsync(d_all_ids + ra.ids_before[rank], d_ids, n_ids * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
  if (n_sentences) HIPG_OR_RETURN(hipMemcpyAsync(d_all_id_offsets + ra.sent_before[rank], d_id_offsets, n_sentences * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
  // ---- rebase ----
  ra.offs = d_all_id_offsets;
  uint64_t grid = (total_s + 1 + 63) / 64;
  if (grid > 2048) grid = 2048;
  HIPG_OR_RETURN(LaunchRebase(ra, static_cast<int>(grid), stream));
  return 0;
}

// ---- the packed gather: 16-bit ids, byte counts, no host synchronisation in the steady state ----
// Transfer: the blocks have ONE size, so an ncclAllGather of bytes would do; the grouped, staggered ncclSend / ncclRecv of
// spmx_all_gather_ids is kept instead -- every rank packs straight into its own slot of the receive array and the unpack
// kernel reads it there, so there is no copy of the rank's own block (an out-of-place all-gather makes one, 1 / world of the
// traffic of a step; an in-place one ties the send buffer to the receive array the same way but leaves the peer order to
// the library), and world - 1 concurrent point-to-point transfers is the pattern a fully connected xGMI node is built for.

uint64_t spmx_packed_block_bytes(uint32_t piece_size, uint64_t max_sentences, uint64_t max_ids, uint64_t max_ids_per_sentence) {
  return MakePackedLayout(piece_size, max_sentences, max_ids, max_ids_per_sentence).bytes;
}

int spmx_pack_ids(const int32_t *d_ids, const uint64_t *d_id_offsets, uint64_t n_sentences, uint32_t piece_size,
                  uint64_t max_sentences, uint64_t max_ids, uint64_t max_ids_per_sentence, uint64_t all_ids_capacity,
                  uint64_t all_offsets_capacity, void *d_block, void *stream) {
  if (!d_block || (reinterpret_cast<uintptr_t>(d_block) & 127u)) return FailG(3, "the block must be device memory aligned to 128 bytes");
  return PackInto(MakePackedLayout(piece_size, max_sentences, max_ids, max_ids_per_sentence), d_ids, d_id_offsets, n_sentences,
                  all_ids_capacity, all_offsets_capacity, static_cast<uint8_t *>(d_block), static_cast<hipStream_t>(stream));
}

int spmx_unpack_ids(const void *d_blocks, int world, uint32_t piece_size, uint64_t max_sentences, uint64_t max_ids,
                    uint64_t max_ids_per_sentence, int32_t *d_all_ids, uint64_t all_ids_capacity, uint64_t *d_all_id_offsets,
                    uint64_t all_offsets_capacity, uint64_t *d_rank_sentences, uint64_t *d_rank_ids, uint64_t *d_status,
                    void *stream) {
  if (world < 1 || world > kMaxRanks) return FailG(3, "world must be 1 .. 64");
  if (!d_blocks || (reinterpret_cast<uintptr_t>(d_blocks) & 127u) || !d_status)
    return FailG(3, "the blocks must be device memory aligned to 128 bytes, the status words not null");
  return UnpackFrom(MakePackedLayout(piece_size, max_sentences, max_ids, max_ids_per_sentence), static_cast<const uint8_t *>(d_blocks),
                    world, d_all_ids, all_ids_capacity, d_all_id_offsets, all_offsets_capacity, d_rank_sentences, d_rank_ids,
                    d_status, static_cast<hipStream_t>(stream));
}

int spmx_packed_status(const uint64_t *status4) {
  if (!status4) return FailG(3, "null status words");
  const int code = static_cast<int>(status4[0]);
  if (code == 0) { t_gather_error.clear(); return 0; }
  return FailG(code, PackedMessage(status4));
}

int spmx_gather_plan_create(void *nccl_comm, int rank, int world, uint32_t piece_size, uint64_t max_sentences,
                            uint64_t max_ids, uint64_t max_ids_per_sentence, spmx_gather_plan **plan) {
  RcclApi &api = Rccl();
  if (!api.ok) return FailG(14, api.error);
  if (world < 1 || world > kMaxRanks || rank < 0 || rank >= world) return FailG(3, "world must be 1 .. 64 and rank inside it");
  if (!nccl_comm || !plan) return FailG(3, "null communicator or plan pointer");
  *plan = nullptr;
  // ---- the agreement: MAX over the ranks, through device memory (the one read-back of this interface) ----
  constexpr int kWords = 4;
  const uint64_t mine[kWords] = {max_sentences, max_ids, max_ids_per_sentence, piece_size};
  uint64_t got[kWords * kMaxRanks];
  uint64_t *d_words = nullptr;
  HIPG_OR_RETURN(hipMalloc(reinterpret_cast<void **>(&d_words), sizeof(uint64_t) * kWords * static_cast<size_t>(1 + world)));
  int rc = 0;
  auto agree = [&]() -> int {
    HIPG_OR_RETURN(hipMemcpyAsync(d_words, mine, sizeof(mine), hipMemcpyHostToDevice, nullptr));
    RCCL_OR_RETURN(api, api.AllGather(d_words, d_words + kWords, kWords, kNcclUint64, nccl_comm, nullptr));
    HIPG_OR_RETURN(hipMemcpyAsync(got, d_words + kWords, sizeof(uint64_t) * kWords * static_cast<size_t>(world), hipMemcpyDeviceToHost, nullptr));
    HIPG_OR_RETURN(hipStreamSynchronize(nullptr));
    return 0;
  };
  rc = agree();
  (void)hipFree(d_words);
  if (rc != 0) return rc;
  uint64_t agreed[kWords] = {0, 0, 0, 0};
  for (int r = 0; r < world; ++r)
    for (int k = 0; k < kWords; ++k)
      if (got[kWords * r + k] > agreed[k]) agreed[k] = got[kWords * r + k];
  spmx_gather_plan *p = new spmx_gather_plan;
  p->comm = nccl_comm;
  p->rank = rank;
  p->world = world;
  p->lay = MakePackedLayout(agreed[3] > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(agreed[3]), agreed[0], agreed[1], agreed[2]);
  auto allocate = [&]() -> int {
    HIPG_OR_RETURN(hipMalloc(reinterpret_cast<void **>(&p->d_blocks), p->lay.bytes * static_cast<size_t>(world)));
    HIPG_OR_RETURN(hipMalloc(reinterpret_cast<void **>(&p->d_status), 4 * sizeof(uint64_t)));
    HIPG_OR_RETURN(hipHostMalloc(reinterpret_cast<void **>(&p->h_status), 4 * sizeof(uint64_t), hipHostMallocDefault));
    HIPG_OR_RETURN(hipMemset(p->d_status, 0, 4 * sizeof(uint64_t)));
    return 0;
  };
  rc = allocate();
  if (rc != 0) { spmx_gather_plan_destroy(p); return rc; }
  *plan = p;
  return 0;
}

uint64_t spmx_gather_plan_block_bytes(const spmx_gather_plan *plan) { return plan ? plan->lay.bytes : 0u; }

int spmx_all_gather_ids_packed(spmx_gather_plan *plan, const int32_t *d_ids, const uint64_t *d_id_offsets,
                               uint64_t n_sentences, int32_t *d_all_ids, uint64_t all_ids_capacity,
                               uint64_t *d_all_id_offsets, uint64_t all_offsets_capacity, uint64_t *d_rank_sentences,
                               uint64_t *d_rank_ids, void *stream_) {
  RcclApi &api = Rccl();
  if (!api.ok) return FailG(14, api.error);
  if (!plan) return FailG(3, "null plan");            // (the only error decided by one rank alone)
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const PackedLayout &lay = plan->lay;
  const int world = plan->world, rank = plan->rank;
  uint8_t *mine = plan->d_blocks + lay.bytes * static_cast<size_t>(rank);
  // Everything a rank could object to -- its shard against the agreed capacities, its ids and counts against the widths, a
  // null buffer, its output capacities -- travels in its block's header, so every rank goes through the same transfers
  // whatever it was given, and every rank's unpack kernel takes the same decision from the same world headers.
  int rc = PackInto(lay, d_ids, d_id_offsets, n_sentences, d_all_ids ? all_ids_capacity : 0u, d_all_id_offsets ? all_offsets_capacity : 0u,
                    mine, stream);
  if (rc != 0) return rc;
  if (world > 1) {
    RCCL_OR_RETURN(api, api.GroupStart());
    int in_group = 0;
    for (int k = 1; k < world && in_group == 0; ++k) {
      const int to = (rank + k) % world, from = (rank - k + world) % world;    // (every rank a different peer per step)
      in_group = api.Send(mine, lay.bytes, kNcclInt8, to, plan->comm, stream);
      if (in_group == 0) in_group = api.Recv(plan->d_blocks + lay.bytes * static_cast<size_t>(from), lay.bytes, kNcclInt8, from, plan->comm, stream);
    }
    const int ended = api.GroupEnd();
    if (in_group != 0) return FailG(13, std::string("ncclSend / ncclRecv: ") + (api.GetErrorString ? api.GetErrorString(in_group) : "RCCL error"));
    RCCL_OR_RETURN(api, ended);
  }
  return UnpackFrom(lay, plan->d_blocks, world, d_all_ids, all_ids_capacity, d_all_id_offsets, all_offsets_capacity, d_rank_sentences,
                    d_rank_ids, plan->d_status, stream);
}

int spmx_gather_plan_status(spmx_gather_plan *plan, void *stream_) {
  if (!plan) return FailG(3, "null plan");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPG_OR_RETURN(hipMemcpyAsync(plan->h_status, plan->d_status, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  HIPG_OR_RETURN(hipStreamSynchronize(stream));
  const int code = static_cast<int>(plan->h_status[0]);
  if (code == 0) { t_gather_error.clear(); return 0; }
  return FailG(code, PackedMessage(plan->h_status));
}

void spmx_gather_plan_destroy(spmx_gather_plan *plan) {
  if (!plan) return;
  (void)hipFree(plan->d_blocks);
  (void)hipFree(plan->d_status);
  if (plan->h_status) (void)hipHostFree(plan->h_status);
  delete plan;
}

}  // extern "C"
