// fpsq_comm.hip.h -- the communicators of a row-sharded handle: the Comm interface; the peer-to-peer route (P2PRoute) and its
// carriers IpcComm (the ranks of a node, hipIpc) and P2PLocalComm (the shards of one process); RcclApi / RcclComm (the library,
// dlopen'ed on first use); LocalGroup / LocalComm (in-process loopback).  Nothing here knows the handle.
// Part of fpsq.hip's translation unit (included through fpsq_handle.hip.h, between DevRgcs and fpsq_solver_s).
#pragma once

#include "fpsq_spmv.hip.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only; the library is dlopen'ed on first use

#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

using namespace fpsq;

namespace {

// ------------------------------------------------------------------ communicators (row-sharded A)
// Collectives are enqueued on the solver's stream; every rank issues the same sequence (the Krylov loop takes
// its exit decision from replicated, bitwise-identical device state at fixed iteration boundaries).
struct Comm {
  int nranks = 1, rank = 0;
  std::string err;
  virtual int allreduce_sum(double* buf, size_t count, hipStream_t s) = 0;
  // Halo mode: vec is this rank's [n_loc][NL] window of raw partial products.  Its first tl rows are the same global
  // columns as the last tl rows of rank - 1's window, its last tr rows the first tr rows of rank + 1's.  On return
  // (stream order) recvL / recvR hold the neighbours' partials on those regions; vec itself is untouched.
  virtual int halo_exchange(const double* vec, int64_t n_loc, int NL, int64_t tl, int64_t tr, double* recvL,
                            double* recvR, hipStream_t s) = 0;
  // recv[r * count + i] = rank r's send[i].  Data movement only: the sums are formed by the step kernel in a fixed
  // rank-major order, so replicated scalars are bitwise identical on every rank by construction.
  virtual int allgather(const double* send, double* recv, size_t count, hipStream_t s) = 0;
  // halo mode, once the handle's exchange buffers exist (collective): a peer-to-peer communicator learns its peers' here
  struct Buffers {
    double* gath[2];      // the two (parity) receive buffers of the all-gathers, [nranks][seg_len] each
    double* halo_recv;    // [(ovl + ovr)][2]
    int64_t ovl, ovr;
  };
  // peer-to-peer routes: the exchange and the finish of the overlap rows as ONE launch (k_p2p_halo_finish); false: not here
  virtual bool halo_exchange_finish(int NL, const HaloFinishArgs& fa, int finish_wgs, hipStream_t s) { return false; }
  // ... and both INSIDE the one-launch iteration (k_iter_fused<.., HALO>): fills the peers' part of the launch's FuseHalo (slots,
  // flag words, the exchange's sequence number); false: this communicator cannot (RCCL: the exchange is a library call)
  virtual bool halo_fused_args(const double* recv, int64_t tl, int64_t tr, FuseHalo& fh) { return false; }
  virtual int arm(const Buffers&, hipStream_t) { return 0; }
  virtual bool failed() { return false; }  // a bounded wait of the peer-to-peer route expired
  // Memory a peer may write into (the gather buffers, the halo slots): a communicator that exports it to other processes
  // or devices decides how it is allocated (fine-grained: visible to a polling kernel across devices).  Freed with hipFree.
  virtual hipError_t alloc_exchange(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  // how the exchanges of the Krylov loop travel (fpsq_info.comm_route)
  virtual int route() const { return FPSQ_ROUTE_RCCL; }
  // Sums over the ranks formed INSIDE the launches that need them (fpsq_krylov.hip.h xch_sum): the device-resident peer table,
  // null when this communicator does not do that (RCCL route; ranks sharing a device).  Known after arm().
  virtual const XchTable* xch_table() const { return nullptr; }
  // ... and the looks the OTHER workgroups of such a launch get beyond kRidePolls (RideArgs::more / FuseArgs::more): they wait for
  // leaders that may be waiting for a late peer, so their bound has to outlast the leaders' (4 x: a follower's look is shorter)
  virtual int wait_more() const { return 0; }
  virtual ~Comm() {}
};

// ---- the peer-to-peer exchange route (halo-sharded loop): NO collective call inside the Krylov loop.  A rank WRITES its
// record straight into its peers' buffers, then its sequence number into their flag words, and waits -- in the same
// one-workgroup kernel, a bounded number of polls -- until its own flag words carry that number (k_p2p_gather, k_p2p_halo).
// Who the peers are is the communicator's business: the other shards of one process (P2PLocalComm: pointers on the same
// device) or the other ranks of a node (IpcComm: their buffers mapped with hipIpcOpenMemHandle; the stores then travel over
// xGMI).  Ordering: gathers alternate between two buffers -- a peer can be at most one reduction ahead, and what it then
// overwrites was consumed before this rank's previous push (which the peer's current one waited for); halo slots alternate
// the same way.
// Every peer table of the peer-to-peer route (here, IpcComm::opened, LocalGroup, P2PPeers in the kernel arguments) has this many
// entries: the GPUs of one node.  More ranks (two nodes, 16 logical ranks) stay on RCCL -- decided in arm(), unanimously.
constexpr int kMaxP2PRanks = 8;
static_assert(sizeof(P2PPeers::rx) / sizeof(double*) == kMaxP2PRanks && sizeof(P2PPeers::flag) / sizeof(unsigned long long*) == kMaxP2PRanks,
              "k_p2p_gather's peer table");
struct P2PRoute {
  int nranks = 1, rank = 0;
  bool armed = false;
  Comm::Buffers mine{};
  // receive area of the all-gathers: [2 parities][rx_half doubles], rx_half >= nranks x the longest record.  The peers write
  // into it; the gather kernel copies what arrived into the handle's ordinary buffer (Buffers::gath), which is what the
  // scalar steps read.  Allocated by the communicator at arm() (exported / fine-grained when the peers are other processes).
  double* rx = nullptr;
  int64_t rx_half = 0;
  double* peer_rx[2][kMaxP2PRanks] = {};
  unsigned long long* peer_flags[kMaxP2PRanks] = {};  // 8 gather words (one per sender), then "from left", "from right"
  double* peer_halo[kMaxP2PRanks] = {};
  int64_t peer_ovl[kMaxP2PRanks] = {}, peer_ovr[kMaxP2PRanks] = {};
  unsigned long long* flags = nullptr;  // mine (device; sequence numbers, monotone); behind the 16 flag words: the receive
                                        // area of the in-launch sums (xch_sum), so that ONE mapped allocation serves both
  static constexpr size_t kFlagWords = 16 + (size_t)kXchRing * kXchRanks * kXchWords;
  XchTable* xt_dev = nullptr;           // non-null: the sums over the ranks are formed inside the launches (lx)
  int lx_want = 1;                      // FPSQ_LX: 0 never, 1 (default) when every rank has a device of its own, 2 always (tests with small grids)
  int xch_delay_rank = 0;               // FPSQ_DEBUG_XCH_DELAY (tests)
  int halo_dbg = 0;                     // HaloFinishArgs::dbg (tests: FPSQ_DEBUG_P2P_DELAY = r + 1)
  int halo_delay_rank = 0;
  int* fail_host = nullptr;             // host-mapped: a bounded wait expired
  int* fail_dev = nullptr;
  unsigned long long gather_seq = 0, halo_seq = 0;
  long max_spins = 50000000L;           // bound of every in-kernel wait (FPSQ_P2P_POLLS; ~1-2 us per poll)
  bool failed() const { return fail_host && *fail_host != 0; }
  int wait_more_dbg = -1;               // FPSQ_DEBUG_WAIT_MORE (tests: 0 = the bound of one GPU)
  int wait_more() const {
    if (wait_more_dbg >= 0) return wait_more_dbg;
    return (int)std::min<long>(4 * std::min<long>(max_spins, (long)INT32_MAX / 8), (long)INT32_MAX / 2);
  }
  int xch_long_delay_ms = 0;            // FPSQ_DEBUG_XCH_LONG_DELAY_MS (tests; with FPSQ_DEBUG_XCH_DELAY naming the rank)
  int alloc_fail_word(std::string& err) {
    if (const char* ev = std::getenv("FPSQ_P2P_POLLS")) max_spins = std::max(1L, std::atol(ev));
    if (const char* ev = std::getenv("FPSQ_HALO_FUSE")) fuse_halo = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("FPSQ_LX")) lx_want = std::atoi(ev);
    if (const char* ev = std::getenv("FPSQ_DEBUG_XCH_DELAY")) xch_delay_rank = std::atoi(ev);
    if (const char* ev = std::getenv("FPSQ_DEBUG_XCH_LONG_DELAY_MS")) xch_long_delay_ms = std::max(0, std::min(2000, std::atoi(ev)));
    if (const char* ev = std::getenv("FPSQ_DEBUG_WAIT_MORE")) wait_more_dbg = std::max(0, std::atoi(ev));
    if (const char* ev = std::getenv("FPSQ_DEBUG_P2P_DELAY")) halo_delay_rank = std::atoi(ev);
    halo_dbg = halo_delay_rank == rank + 1 ? 1 : 0;
    if (hipHostMalloc((void**)&fail_host, 4, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void**)&fail_dev, fail_host, 0) != hipSuccess) {
      err = "p2p arm: allocation failed";
      return FPSQ_ERR_HIP;
    }
    *fail_host = 0;
    return 0;
  }
  // the peer table of the in-launch sums, once peer_flags[] is known
  int make_xch_table(std::string& err) {
    XchTable T{};
    for (int r = 0; r < nranks; ++r) T.peer[r] = peer_flags[r] + 16;
    T.nranks = nranks;
    T.rank = rank;
    T.max_polls = (int32_t)std::min<long>(max_spins, (long)INT32_MAX);
    T.delay_rank = xch_delay_rank;
    T.long_delay_ticks = (unsigned int)xch_long_delay_ms * 100000u;  // (100 MHz)
    T.fail = fail_dev;
    if (hipMalloc((void**)&xt_dev, sizeof(XchTable)) != hipSuccess ||
        hipMemcpy(xt_dev, &T, sizeof T, hipMemcpyHostToDevice) != hipSuccess) {
      err = "p2p arm: allocation failed";
      return FPSQ_ERR_HIP;
    }
    return 0;
  }
  bool is_gather_buffer(const double* recv) const { return armed && (recv == mine.gath[0] || recv == mine.gath[1]); }
  void allgather(const double* send, double* recv, size_t count, hipStream_t s) {
    const int par = recv == mine.gath[1];
    P2PPeers P{};
    P.n = nranks;
    for (int r = 0; r < nranks; ++r) {
      P.rx[r] = peer_rx[par][r];
      P.flag[r] = peer_flags[r];
    }
    // (a long record -- few ranks, many row blocks each -- gets extra workgroups for the copy of the rank's own part)
    const int extra = (int)std::min<size_t>(7, count / (8 * kBlock));
    hipLaunchKernelGGL(k_p2p_gather, dim3(nranks + extra), dim3(kBlock), 0, s, send, (int64_t)count, P, rank, ++gather_seq,
                       rx + (size_t)par * rx_half, recv, fail_dev, max_spins);
  }
  void halo_exchange(const double* vec, int NL, int64_t tl, int64_t tr, const double* recvL, hipStream_t s) {
    const P2PHalo H = halo_peers(NL, tl, tr, recvL);
    hipLaunchKernelGGL(k_p2p_halo, dim3(2), dim3(1024), 0, s, vec, tl * NL, tr * NL, H, ++halo_seq, fail_dev, max_spins);
  }
  P2PHalo halo_peers(int NL, int64_t tl, int64_t tr, const double* recvL) const {
    P2PHalo H{};
    const int par = recvL != mine.halo_recv;  // which half of the (double-buffered) slots this exchange uses: the same on
                                              // every rank (all ranks make the same sequence of exchanges)
    if (rank > 0 && tl > 0) {  // my head region = the left neighbour's tail slot (behind its own head slot)
      const int L = rank - 1;
      H.left_dst = peer_halo[L] + (size_t)par * (size_t)(peer_ovl[L] + peer_ovr[L]) * 2 + (size_t)peer_ovl[L] * NL;
      H.left_flag = peer_flags[L] + 9;  // its "from right" word
      H.my_from_left = flags + 8;
    }
    if (rank < nranks - 1 && tr > 0) {
      const int R = rank + 1;
      H.right_dst = peer_halo[R] + (size_t)par * (size_t)(peer_ovl[R] + peer_ovr[R]) * 2;
      H.right_flag = peer_flags[R] + 8;  // its "from left" word
      H.my_from_right = flags + 9;
    }
    return H;
  }
  bool fuse_halo = true;  // FPSQ_HALO_FUSE=0: exchange and finish as two launches
  bool halo_fused_args(const double* recv, int64_t tl, int64_t tr, FuseHalo& fh) {
    if (!armed) return false;
    fh.H = halo_peers(2, tl, tr, recv);
    fh.seq = ++halo_seq;
    fh.fail = fail_dev;
    fh.max_spins = max_spins;
    fh.arrive = flags + 12;
    return true;
  }
  bool halo_exchange_finish(int NL, const HaloFinishArgs& fa, int finish_wgs, hipStream_t s) {
    if (!armed || !fuse_halo) return false;
    const P2PHalo H = halo_peers(NL, fa.tl, fa.tr, fa.recv);
    const dim3 grid(2 * kHaloCopy + finish_wgs);
    unsigned long long* arrive = flags + 12;  // (words 12, 13 of my flag block: arrival counters of the copy slices, per side)
    HaloFinishArgs fb = fa;
    fb.dbg = halo_dbg;
    if (NL == 2)
      hipLaunchKernelGGL(k_p2p_halo_finish<2>, grid, dim3(kBlock), 0, s, H, ++halo_seq, fail_dev, max_spins, arrive, fb);
    else
      hipLaunchKernelGGL(k_p2p_halo_finish<1>, grid, dim3(kBlock), 0, s, H, ++halo_seq, fail_dev, max_spins, arrive, fb);
    return true;
  }
  void release() {
    if (xt_dev) hipFree(xt_dev);
    xt_dev = nullptr;
    if (rx) hipFree(rx);
    rx = nullptr;
    if (flags) hipFree(flags);
    if (fail_host) hipHostFree(fail_host);
    flags = nullptr;
    fail_host = nullptr;
  }
};

struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  bool load(std::string& err) {
    if (lib) return true;
    // by SONAME first: a process that imported torch already holds librccl.so.1 and must keep using that copy
    // FPSQ_RCCL_LIB: another build of the collectives library (a site build; the multi-process loopback stand-in of
    // tests/shim, which lets the multi-rank path run on a one-GPU box) -- then that one or nothing
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    if (const char* ov = std::getenv("FPSQ_RCCL_LIB")) {
      lib = dlopen(ov, RTLD_NOW | RTLD_LOCAL);
    } else {
      for (const char* nm : names)
        if ((lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL))) break;
    }
    if (!lib) {
      err = std::string("cannot dlopen librccl: ") + dlerror();
      return false;
    }
    GetUniqueId = (decltype(GetUniqueId))dlsym(lib, "ncclGetUniqueId");
    CommInitRank = (decltype(CommInitRank))dlsym(lib, "ncclCommInitRank");
    AllReduce = (decltype(AllReduce))dlsym(lib, "ncclAllReduce");
    AllGather = (decltype(AllGather))dlsym(lib, "ncclAllGather");
    CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
    GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
    Send = (decltype(Send))dlsym(lib, "ncclSend");
    Recv = (decltype(Recv))dlsym(lib, "ncclRecv");
    GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart");
    GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd");
    if (!GetUniqueId || !CommInitRank || !AllReduce || !AllGather || !CommDestroy || !GetErrorString || !Send || !Recv || !GroupStart ||
        !GroupEnd) {
      err = "librccl is missing a required symbol";
      return false;
    }
    return true;
  }
};
RcclApi g_rccl;

struct RcclComm : Comm {
  ncclComm_t c = nullptr;
  int allreduce_sum(double* buf, size_t count, hipStream_t s) override {
    ncclResult_t r = g_rccl.AllReduce(buf, buf, count, ncclDouble, ncclSum, c, s);
    if (r != ncclSuccess) {
      err = std::string("ncclAllReduce: ") + g_rccl.GetErrorString(r);
      return FPSQ_ERR_COMM;
    }
    return 0;
  }
  int allgather(const double* send, double* recv, size_t count, hipStream_t s) override {
    ncclResult_t r = g_rccl.AllGather(send, recv, count, ncclDouble, c, s);
    if (r != ncclSuccess) {
      err = std::string("ncclAllGather: ") + g_rccl.GetErrorString(r);
      return FPSQ_ERR_COMM;
    }
    return 0;
  }
  // neighbour-to-neighbour exchange over xGMI: one grouped send/recv pair per neighbour (<= 2 x window x NL doubles)
  int halo_exchange(const double* vec, int64_t n_loc, int NL, int64_t tl, int64_t tr, double* recvL, double* recvR,
                    hipStream_t s) override {
    ncclResult_t r = g_rccl.GroupStart();
    if (r == ncclSuccess && rank > 0 && tl > 0) {
      r = g_rccl.Send(vec, (size_t)tl * NL, ncclDouble, rank - 1, c, s);
      if (r == ncclSuccess) r = g_rccl.Recv(recvL, (size_t)tl * NL, ncclDouble, rank - 1, c, s);
    }
    if (r == ncclSuccess && rank < nranks - 1 && tr > 0) {
      r = g_rccl.Send(vec + (size_t)(n_loc - tr) * NL, (size_t)tr * NL, ncclDouble, rank + 1, c, s);
      if (r == ncclSuccess) r = g_rccl.Recv(recvR, (size_t)tr * NL, ncclDouble, rank + 1, c, s);
    }
    const ncclResult_t e = g_rccl.GroupEnd();
    if (r == ncclSuccess) r = e;
    if (r != ncclSuccess) {
      err = std::string("halo exchange (ncclSend/ncclRecv): ") + g_rccl.GetErrorString(r);
      return FPSQ_ERR_COMM;
    }
    return 0;
  }
  ~RcclComm() override {
    if (c) g_rccl.CommDestroy(c);
  }
};

// The ranks of ONE NODE, one process per GPU: RCCL for the set-up collectives and as the fallback, the peer-to-peer route
// (P2PRoute) for the exchanges of the halo-sharded Krylov loop.  At arm() every rank exports its two gather buffers, its
// halo slots and its flag words with hipIpcGetMemHandle, the handles travel through one RCCL all-gather, every rank maps
// its peers' with hipIpcOpenMemHandle (peer access enabled lazily: the stores of k_p2p_gather / k_p2p_halo then go over
// xGMI), and a second all-gather makes the decision unanimous: if ANY rank could not export or open, all stay on RCCL.
// At the headline size the RCCL route pays three collective calls (15-30 us each) per joint iteration against ~8 us of
// products on 8 GPUs; this one pays three one-workgroup kernels.  IPC handles open between processes sharing ONE device
// too, which is how the route is tested here (tests/test_gpu_p2p_ipc.py: 2 and 3 processes on one GPU).
struct IpcComm : RcclComm {
  int want = FPSQ_ROUTE_AUTO;   // fpsq_comm_set_route / FPSQ_COMM_ROUTE
  P2PRoute rt;
  std::string note;             // why the route fell back to RCCL (fpsq_last_error after a FPSQ_ROUTE_P2P request)
  void* opened[kMaxP2PRanks][3] = {};
  struct Blob {                 // what a rank tells its peers (padded to whole doubles)
    hipIpcMemHandle_t h[3];     // receive area of the gathers (one allocation, both parities), halo slots, flag words
    int64_t ovl, ovr, rx_half;  // rx_half: doubles between the two parities of the receive area
    int32_t ok, pid;
    int32_t lx_want, pad;       // FPSQ_LX of that rank (the in-launch sums are switched on unanimously)
    char dev[48];               // PCI bus id of its device: two ranks on ONE device keep the exchange kernels (see xch_sum)
  };
  static constexpr size_t kBlobDoubles = (sizeof(Blob) + 7) / 8;
  hipError_t alloc_exchange(void** p, size_t bytes) override {
    if (want == FPSQ_ROUTE_RCCL) return hipMalloc(p, bytes);
    // fine-grained: a peer's stores must become visible to a kernel of this device that is polling / about to read
    hipError_t e = hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      e = hipMalloc(p, bytes);
    }
    return e;
  }
  int route() const override { return rt.armed ? FPSQ_ROUTE_P2P : FPSQ_ROUTE_RCCL; }
  const XchTable* xch_table() const override { return rt.armed ? rt.xt_dev : nullptr; }
  int wait_more() const override { return rt.armed && rt.xt_dev ? rt.wait_more() : 0; }
  bool failed() override { return rt.failed(); }
  int arm(const Buffers& b, hipStream_t s) override {
    if (want == FPSQ_ROUTE_RCCL) return 0;
    if (nranks > kMaxP2PRanks) {  // (every rank sees the same nranks: the same decision everywhere, no exchange needed)
      note = "more than " + std::to_string(kMaxP2PRanks) + " ranks: the peer tables of the peer-to-peer route hold one node's GPUs";
      if (want == FPSQ_ROUTE_P2P) {
        err = "peer-to-peer route requested but not available: " + note;
        return FPSQ_ERR_COMM;
      }
      return 0;
    }
    rt.nranks = nranks;
    rt.rank = rank;
    rt.mine = b;
    Blob me{};
    me.ok = 1;
    me.pid = (int32_t)getpid();
    me.ovl = b.ovl;
    me.ovr = b.ovr;
    rt.rx_half = b.gath[1] - b.gath[0];
    me.rx_half = rt.rx_half;
    if (hipExtMallocWithFlags((void**)&rt.flags, P2PRoute::kFlagWords * 8, hipDeviceMallocFinegrained) != hipSuccess ||
        hipExtMallocWithFlags((void**)&rt.rx, (size_t)rt.rx_half * 2 * 8, hipDeviceMallocFinegrained) != hipSuccess) {
      (void)hipGetLastError();
      if (rt.flags) hipFree(rt.flags);
      rt.flags = nullptr;
      rt.rx = nullptr;
      me.ok = 0;
      note = "fine-grained allocation of the flag words / receive area failed";
      // (the kernels are never launched without them: the route stays unarmed)
    } else {
      hipMemset(rt.flags, 0, P2PRoute::kFlagWords * 8);
    }
    if (int rc = rt.alloc_fail_word(err)) return rc;
    me.lx_want = rt.lx_want;
    {
      int dev = 0;
      if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetPCIBusId(me.dev, (int)sizeof me.dev, dev) != hipSuccess) {
        (void)hipGetLastError();
        std::snprintf(me.dev, sizeof me.dev, "?");  // (unknown: counts as shared)
      }
    }
    if (me.ok && nranks > 1) {
      void* base[3] = {rt.rx, b.halo_recv, rt.flags};
      for (int k = 0; k < 3 && me.ok; ++k)
        if (hipIpcGetMemHandle(&me.h[k], base[k]) != hipSuccess) {
          (void)hipGetLastError();
          me.ok = 0;
          note = "hipIpcGetMemHandle failed";
        }
    }
    hipDeviceSynchronize();
    // round 1: everybody's blob
    std::vector<double> all(kBlobDoubles * nranks), mine_d(kBlobDoubles, 0.0);
    std::memcpy(mine_d.data(), &me, sizeof me);
    double *dsend = nullptr, *drecv = nullptr;
    if (hipMalloc((void**)&dsend, kBlobDoubles * 8) != hipSuccess || hipMalloc((void**)&drecv, all.size() * 8) != hipSuccess) {
      err = "p2p arm: allocation failed";
      return FPSQ_ERR_HIP;
    }
    auto gather_round = [&](const std::vector<double>& snd, size_t cnt) -> int {
      if (hipMemcpyAsync(dsend, snd.data(), cnt * 8, hipMemcpyHostToDevice, s) != hipSuccess) return FPSQ_ERR_HIP;
      if (int rc = RcclComm::allgather(dsend, drecv, cnt, s)) return rc;
      if (hipMemcpyAsync(all.data(), drecv, cnt * nranks * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipStreamSynchronize(s) != hipSuccess)
        return FPSQ_ERR_HIP;
      return 0;
    };
    int rc = gather_round(mine_d, kBlobDoubles);
    std::vector<Blob> blobs(nranks);
    bool ok = rc == 0;
    if (rc == 0) {
      for (int r = 0; r < nranks; ++r) {
        std::memcpy(&blobs[r], all.data() + kBlobDoubles * r, sizeof(Blob));
        if (!blobs[r].ok) {
          ok = false;
          if (note.empty()) note = "rank " + std::to_string(r) + " could not export its buffers";
        }
      }
    }
    // map the peers' buffers
    if (ok) {
      for (int r = 0; r < nranks && ok; ++r) {
        if (r == rank) continue;
        for (int k = 0; k < 3 && ok; ++k)
          if (hipIpcOpenMemHandle(&opened[r][k], blobs[r].h[k], hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
            (void)hipGetLastError();
            opened[r][k] = nullptr;
            ok = false;
            note = "hipIpcOpenMemHandle failed for rank " + std::to_string(r) +
                   (blobs[r].pid == me.pid ? " (same process: use the in-process group instead)" : "");
          }
      }
    }
    // round 2: unanimous or not at all
    if (rc == 0) {
      std::vector<double> v(1, ok ? 1.0 : 0.0);
      rc = gather_round(v, 1);
      if (rc == 0)
        for (int r = 0; r < nranks; ++r)
          if (all[r] == 0.0) {
            if (ok && note.empty()) note = "rank " + std::to_string(r) + " could not map its peers' buffers";
            ok = false;
          }
    }
    hipFree(dsend);
    hipFree(drecv);
    if (rc) return rc;
    if (!ok) {
      close_peers();
      if (want == FPSQ_ROUTE_P2P) {
        err = "peer-to-peer route requested but not available: " + note;
        return FPSQ_ERR_COMM;
      }
      return 0;  // (every rank took the same decision: the RCCL route)
    }
    for (int r = 0; r < nranks; ++r) {
      const bool self = r == rank;
      double* g0 = self ? rt.rx : (double*)opened[r][0];
      rt.peer_rx[0][r] = g0;
      rt.peer_rx[1][r] = g0 + blobs[r].rx_half;
      rt.peer_halo[r] = self ? b.halo_recv : (double*)opened[r][1];
      rt.peer_flags[r] = self ? rt.flags : (unsigned long long*)opened[r][2];
      rt.peer_ovl[r] = blobs[r].ovl;
      rt.peer_ovr[r] = blobs[r].ovr;
    }
    // In-launch sums over the ranks (xch_sum): every rank must want them, and either every rank has a device of its own or every
    // rank forces them (FPSQ_LX=2: tests whose grids are resident all at once).  Every rank sees the same blobs: same decision.
    {
      bool all_on = true, all_force = true, distinct = true;
      for (int r = 0; r < nranks; ++r) {
        all_on = all_on && blobs[r].lx_want >= 1;
        all_force = all_force && blobs[r].lx_want >= 2;
        for (int q = 0; q < r; ++q)
          if (std::strncmp(blobs[r].dev, blobs[q].dev, sizeof blobs[r].dev) == 0 || blobs[r].dev[0] == '?') distinct = false;
      }
      if (nranks > 1 && all_on && (distinct || all_force))
        if (int rc2 = rt.make_xch_table(err)) return rc2;
    }
    rt.armed = true;
    return 0;
  }
  int allgather(const double* send, double* recv, size_t count, hipStream_t s) override {
    if (!rt.is_gather_buffer(recv)) return RcclComm::allgather(send, recv, count, s);
    rt.allgather(send, recv, count, s);
    return 0;
  }
  int halo_exchange(const double* vec, int64_t n_loc, int NL, int64_t tl, int64_t tr, double* recvL, double* recvR,
                    hipStream_t s) override {
    if (!rt.armed) return RcclComm::halo_exchange(vec, n_loc, NL, tl, tr, recvL, recvR, s);
    rt.halo_exchange(vec, NL, tl, tr, recvL, s);
    return 0;
  }
  bool halo_exchange_finish(int NL, const HaloFinishArgs& fa, int finish_wgs, hipStream_t s) override {
    return rt.halo_exchange_finish(NL, fa, finish_wgs, s);
  }
  bool halo_fused_args(const double* recv, int64_t tl, int64_t tr, FuseHalo& fh) override { return rt.halo_fused_args(recv, tl, tr, fh); }
  void close_peers() {
    for (int r = 0; r < kMaxP2PRanks; ++r)
      for (int k = 0; k < 3; ++k)
        if (opened[r][k]) {
          hipIpcCloseMemHandle(opened[r][k]);
          opened[r][k] = nullptr;
        }
  }
  ~IpcComm() override {
    close_peers();
    rt.release();
  }
};

// P logical shards in ONE process on ONE device (each handle driven by its own host thread): the sum is a kernel.
struct LocalGroup {
  int n = 0;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  long generation = 0;
  double* bufs[8] = {};
  const double* vecs[8] = {};  // halo exchange: every shard's window of partial products and its length
  int64_t nloc[8] = {};
  hipEvent_t ready[8] = {};
  hipEvent_t copied[8] = {};
  hipEvent_t done = nullptr;
  // peer-to-peer route (fpsq_local_group_set_p2p): what every shard published at arm()
  bool p2p = false;
  struct Pub {
    double* rx[2];
    unsigned long long* flags;  // 8 gather flag words (one per sender), then "from left", "from right"
    double* halo_recv;
    int64_t ovl, ovr;
  } pub[8] = {};
  void barrier() {
    std::unique_lock<std::mutex> lk(mu);
    const long gen = generation;
    if (++arrived == n) {
      arrived = 0;
      ++generation;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return generation != gen; });
    }
  }
};

struct LocalComm : Comm {
  LocalGroup* g = nullptr;
  int route() const override { return FPSQ_ROUTE_LOCAL; }
  int allreduce_sum(double* buf, size_t count, hipStream_t s) override {
    g->bufs[rank] = buf;
    hipEventRecord(g->ready[rank], s);
    g->barrier();
    if (rank == 0) {
      ShardBufs B;
      B.n = g->n;
      for (int r = 0; r < g->n; ++r) {
        hipStreamWaitEvent(s, g->ready[r], 0);
        B.b[r] = g->bufs[r];
      }
      const int grid = (int)std::max<size_t>(1, std::min<size_t>((count + kBlock - 1) / kBlock, 2048));
      hipLaunchKernelGGL(k_local_allreduce, dim3(grid), dim3(kBlock), 0, s, B, (int64_t)count);
      hipEventRecord(g->done, s);
    }
    g->barrier();
    hipStreamWaitEvent(s, g->done, 0);
    g->barrier();  // nobody may start the next collective (and overwrite bufs[] / re-record events) before all queued the wait
    return 0;
  }
  int allgather(const double* send, double* recv, size_t count, hipStream_t s) override {
    g->vecs[rank] = send;
    hipEventRecord(g->ready[rank], s);
    g->barrier();  // every shard's source pointer and `ready` event are published
    GatherSrc S;
    S.n = g->n;
    for (int r = 0; r < g->n; ++r) {
      if (r != rank) hipStreamWaitEvent(s, g->ready[r], 0);
      S.s[r] = g->vecs[r];
    }
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((count * g->n + kBlock - 1) / kBlock, 256));
    hipLaunchKernelGGL(k_local_allgather, dim3(grid), dim3(kBlock), 0, s, S, recv, (int64_t)count);
    hipEventRecord(g->copied[rank], s);
    g->barrier();  // every `copied` event is recorded
    // a shard's next kernels rewrite its source array: every other shard must have taken its copy first
    for (int r = 0; r < g->n; ++r)
      if (r != rank) hipStreamWaitEvent(s, g->copied[r], 0);
    g->barrier();  // the events may be re-recorded by the next collective only after everyone queued its waits
    return 0;
  }
  int halo_exchange(const double* vec, int64_t n_loc, int NL, int64_t tl, int64_t tr, double* recvL, double* recvR,
                    hipStream_t s) override {
    g->vecs[rank] = vec;
    g->nloc[rank] = n_loc;
    hipEventRecord(g->ready[rank], s);
    g->barrier();  // every shard's pointer and `ready` event are published
    if (rank > 0 && tl > 0) {
      hipStreamWaitEvent(s, g->ready[rank - 1], 0);
      hipMemcpyAsync(recvL, g->vecs[rank - 1] + (size_t)(g->nloc[rank - 1] - tl) * NL, (size_t)tl * NL * 8,
                     hipMemcpyDeviceToDevice, s);
    }
    if (rank < nranks - 1 && tr > 0) {
      hipStreamWaitEvent(s, g->ready[rank + 1], 0);
      hipMemcpyAsync(recvR, g->vecs[rank + 1], (size_t)tr * NL * 8, hipMemcpyDeviceToDevice, s);
    }
    hipEventRecord(g->copied[rank], s);
    g->barrier();  // every `copied` event is recorded
    // the caller's next kernel modifies vec: both neighbours must have taken their copies of it first
    if (rank > 0) hipStreamWaitEvent(s, g->copied[rank - 1], 0);
    if (rank < nranks - 1) hipStreamWaitEvent(s, g->copied[rank + 1], 0);
    g->barrier();  // the events may be re-recorded by the next collective only after everyone queued its waits
    return 0;
  }
};

// The same logical shards on the peer-to-peer route (P2PRoute): the peers are the other shards' buffers on the same
// device, which exercises the protocol (ordering, double buffering, bounded waits), not a link.  Set-up collectives
// (before arm()) use LocalComm's.
struct P2PLocalComm : LocalComm {
  P2PRoute rt;
  int route() const override { return FPSQ_ROUTE_LOCAL_P2P; }
  const XchTable* xch_table() const override { return rt.armed ? rt.xt_dev : nullptr; }
  int wait_more() const override { return rt.armed && rt.xt_dev ? rt.wait_more() : 0; }
  int arm(const Buffers& b, hipStream_t) override {
    rt.nranks = nranks;
    rt.rank = rank;
    rt.mine = b;
    rt.rx_half = b.gath[1] - b.gath[0];
    if (hipMalloc((void**)&rt.flags, P2PRoute::kFlagWords * 8) != hipSuccess ||
        hipMemset(rt.flags, 0, P2PRoute::kFlagWords * 8) != hipSuccess ||
        hipMalloc((void**)&rt.rx, (size_t)rt.rx_half * 2 * 8) != hipSuccess) {
      err = "p2p arm: allocation failed";
      return FPSQ_ERR_HIP;
    }
    if (int rc = rt.alloc_fail_word(err)) return rc;
    hipDeviceSynchronize();
    LocalGroup::Pub& me = g->pub[rank];
    me.rx[0] = rt.rx;
    me.rx[1] = rt.rx + rt.rx_half;
    me.flags = rt.flags;
    me.halo_recv = b.halo_recv;
    me.ovl = b.ovl;
    me.ovr = b.ovr;
    g->barrier();  // every shard has published
    for (int r = 0; r < nranks; ++r) {
      const LocalGroup::Pub& q = g->pub[r];
      rt.peer_rx[0][r] = q.rx[0];
      rt.peer_rx[1][r] = q.rx[1];
      rt.peer_flags[r] = q.flags;
      rt.peer_halo[r] = q.halo_recv;
      rt.peer_ovl[r] = q.ovl;
      rt.peer_ovr[r] = q.ovr;
    }
    // (the shards share ONE device: the in-launch sums only when a test with small grids forces them -- one environment, one decision)
    if (nranks > 1 && rt.lx_want >= 2)
      if (int rc = rt.make_xch_table(err)) return rc;
    rt.armed = true;
    g->barrier();
    return 0;
  }
  bool failed() override { return rt.failed(); }
  int allgather(const double* send, double* recv, size_t count, hipStream_t s) override {
    if (!rt.is_gather_buffer(recv)) return LocalComm::allgather(send, recv, count, s);
    rt.allgather(send, recv, count, s);
    return 0;
  }
  int halo_exchange(const double* vec, int64_t n_loc, int NL, int64_t tl, int64_t tr, double* recvL, double* recvR,
                    hipStream_t s) override {
    if (!rt.armed) return LocalComm::halo_exchange(vec, n_loc, NL, tl, tr, recvL, recvR, s);
    rt.halo_exchange(vec, NL, tl, tr, recvL, s);
    return 0;
  }
  bool halo_exchange_finish(int NL, const HaloFinishArgs& fa, int finish_wgs, hipStream_t s) override {
    return rt.halo_exchange_finish(NL, fa, finish_wgs, s);
  }
  bool halo_fused_args(const double* recv, int64_t tl, int64_t tr, FuseHalo& fh) override { return rt.halo_fused_args(recv, tl, tr, fh); }
  ~P2PLocalComm() override { rt.release(); }
};

}  // namespace
