// vv_exchange.cpp -- between the ranks of a sharded run: the RCCL communicator (loaded at run time) and the xGMI mailbox.
#include "vv_plan.hpp"

#include <dlfcn.h>

RcclApi& rccl_api() {
    static RcclApi r;
    if (r.handle) return r;
    r.handle = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!r.handle) r.handle = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!r.handle) r.handle = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!r.handle) return r;
    r.getUniqueId = (decltype(r.getUniqueId)) dlsym(r.handle, "ncclGetUniqueId");
    r.commInitRank = (decltype(r.commInitRank)) dlsym(r.handle, "ncclCommInitRank");
    r.allReduce = (decltype(r.allReduce)) dlsym(r.handle, "ncclAllReduce");
    r.commDestroy = (decltype(r.commDestroy)) dlsym(r.handle, "ncclCommDestroy");
    r.commCount = (decltype(r.commCount)) dlsym(r.handle, "ncclCommCount");
    r.getErrorString = (decltype(r.getErrorString)) dlsym(r.handle, "ncclGetErrorString");
    r.ok = r.getUniqueId && r.commInitRank && r.allReduce && r.commDestroy;
    return r;
}

// Element-wise int64 sum of the accumulators of `phase` over all ranks, on the plan's stream (ncclSum is exact on
// integers, so every rank continues with identical bits).  No-op without a communicator.
int exchange_accumulators(vvhip_plan* p, int phase) {
    if (use_mailbox(p)) return VVHIP_OK;   // kernel B exchanges the totals itself
    if (!p->comm) return VVHIP_OK;      // a 1-rank communicator still issues the collective (exercises the path on one GPU)
    void* ptr = nullptr;
    int32_t count = 0;
    int rc = vvhip_accumulators(p, phase, &ptr, &count);
    if (rc != VVHIP_OK) return rc;
    ScopedTimer t(p, T_OTHER);
    ncclResult_t e = rccl_api().allReduce(ptr, ptr, (size_t) count, ncclInt64, ncclSum, p->comm, p->stream);
    if (e != ncclSuccess) return fail(p, VVHIP_ERR_HIP, std::string("ncclAllReduce: ") + (rccl_api().getErrorString ? rccl_api().getErrorString(e) : "error"));
    return VVHIP_OK;
}

// ---- xGMI mailbox (include/vvhip.h): create -> exchange the 64-byte handles by any means -> connect
// back to "created, not connected": the peers' mappings and the table of them go
static void mailbox_disconnect(vvhip_plan* p) {
    p->mb_on = false;
    p->mb_shared_device = false;       // (a second connect must not count the first one's ranks again)
    p->mb_device_ranks = 1;
    p->mb_opened.clear();
    p->d_mb_peers.reset();
}
void mailbox_release(vvhip_plan* p) {
    mailbox_disconnect(p);
    p->d_mb_ctl.reset();
    p->mb_local.reset();
    p->mb_ranks = 0;
}

extern "C" {

int vvhip_comm_unique_id(void* id128) {
    if (!id128) return VVHIP_ERR_INVALID;
    RcclApi& r = rccl_api();
    if (!r.ok) return VVHIP_ERR_UNSUPPORTED;
    ncclUniqueId id;
    if (r.getUniqueId(&id) != ncclSuccess) return VVHIP_ERR_HIP;
    std::memcpy(id128, &id, sizeof(id));
    return VVHIP_OK;
}
int vvhip_comm_init(vvhip_plan* p, const void* id128, int nranks, int rank) {
    NEED_BOUND(p);
    if (!id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(p, VVHIP_ERR_INVALID, "bad communicator arguments");
    RcclApi& r = rccl_api();
    if (!r.ok) return fail(p, VVHIP_ERR_UNSUPPORTED, "librccl.so.1 could not be loaded");
    if (p->comm) { (void) r.commDestroy(p->comm); p->comm = nullptr; }
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    ncclResult_t e = r.commInitRank(&p->comm, nranks, id, rank);
    if (e != ncclSuccess) { p->comm = nullptr; return fail(p, VVHIP_ERR_HIP, std::string("ncclCommInitRank: ") + (r.getErrorString ? r.getErrorString(e) : "error")); }
    p->comm_ranks = nranks;
    drop_graphs(p);
    return VVHIP_OK;
}
int vvhip_comm_count(vvhip_plan* p, int32_t* ranks) {
    if (!p || !ranks) return VVHIP_ERR_INVALID;
    *ranks = 0;
    if (!p->comm) return VVHIP_OK;                   // no communicator: 0
    RcclApi& r = rccl_api();
    int n = p->comm_ranks;
    if (r.commCount && r.commCount(p->comm, &n) != ncclSuccess) return fail(p, VVHIP_ERR_HIP, "ncclCommCount failed");
    *ranks = n;
    return VVHIP_OK;
}
int vvhip_peer_access(int device, int peer_device, int32_t* can_access) {
    if (!can_access) return VVHIP_ERR_INVALID;
    int can = 0;
    if (device == peer_device) { *can_access = 1; return VVHIP_OK; }
    if (hipDeviceCanAccessPeer(&can, device, peer_device) != hipSuccess) return VVHIP_ERR_HIP;
    *can_access = can;
    return VVHIP_OK;
}
int vvhip_mailbox_create(vvhip_plan* p, int nranks, int rank, void* handle64) {
    NEED_BOUND(p);
    if (!handle64 || nranks < 1 || nranks > vv::MB_MAX_RANKS || rank < 0 || rank >= nranks)
        return fail(p, VVHIP_ERR_INVALID, "mailbox: 1 <= ranks <= 16, 0 <= rank < ranks");
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "the C ABI hands the IPC handle over as 64 bytes");
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    mailbox_release(p);
    drop_graphs(p);
    const size_t bytes = (size_t) 2 * nranks * vv::MB_WORDS * sizeof(unsigned long long);
    // uncached: peers' stores land in this GPU's memory over xGMI and must be seen by loads that would otherwise hit in L2
    HIP_TRY(p, vv::zeros(p->mb_local, std::max(bytes, (size_t) 4096), p->stream, true));
    HIP_TRY(p, vv::zeros(p->d_mb_ctl, 4 * sizeof(unsigned int), p->stream));
    HIP_TRY(p, hipDeviceSynchronize());
    hipIpcMemHandle_t h;
    HIP_TRY(p, hipIpcGetMemHandle(&h, p->mb_local.get()));
    std::memcpy(handle64, &h, 64);
    p->mb_ranks = nranks;
    p->mb_rank = rank;
    return VVHIP_OK;
}
int vvhip_mailbox_connect(vvhip_plan* p, const void* handles) {
    NEED_BOUND(p);
    if (!p->mb_local || !handles) return fail(p, VVHIP_ERR_INVALID, "vvhip_mailbox_create has not been called");
    std::vector<unsigned long long*> peers((size_t) p->mb_ranks, nullptr);
    // A second connect: what vvhip_mailbox_destroy does first -- captured step graphs carry the OLD peer table's address and the peers' box
    // addresses in their kernel arguments (a replay after the free below would read unmapped memory), launches still in flight use them too,
    // and whether the step may be one launch depends on who shares the device (re-evaluated: forget_fused_checks).
    TRY(settle_recovery(p));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    drop_graphs(p);
    forget_fused_checks(p);
    mailbox_disconnect(p);
    // (an error below leaves the mailbox as it is now: created, not connected)
    auto give_up = [p](hipError_t e, const char* what) { mailbox_disconnect(p); return hip_fail(p, e, what); };
    for (int r = 0; r < p->mb_ranks; r++) {
        if (r == p->mb_rank) { peers[r] = p->mb_local.get(); continue; }
        hipIpcMemHandle_t h;
        std::memcpy(&h, (const char*) handles + (size_t) r * 64, 64);
        vv::IpcMapping box;
        if (hipError_t e = box.open(h); e != hipSuccess) return give_up(e, "hipIpcOpenMemHandle");
        void* m = box.get();
        p->mb_opened.push_back(std::move(box));
        peers[r] = (unsigned long long*) m;
        // whose memory is it?  A box on this very device means that rank shares the GPU with this one
        hipPointerAttribute_t attr;
        int dev = -1;
        if (hipGetDevice(&dev) == hipSuccess && hipPointerGetAttributes(&attr, m) == hipSuccess && attr.device == dev) { p->mb_shared_device = true; p->mb_device_ranks++; }
        else (void) hipGetLastError();
    }
    if (hipError_t e = vv::upload(p->d_mb_peers, peers); e != hipSuccess) return give_up(e, "upload of the peer table");
    p->mb_on = true;
    return VVHIP_OK;
}
int vvhip_mailbox_status(vvhip_plan* p, int32_t* active, int32_t* timed_out) {
    NEED_BOUND(p);
    if (active) *active = use_mailbox(p) ? 1 : 0;
    if (timed_out) {
        *timed_out = 0;
        if (p->d_mb_ctl) {
            unsigned int ctl[4];
            HIP_TRY(p, hipStreamSynchronize(p->stream));
            HIP_TRY(p, hipMemcpy(ctl, p->d_mb_ctl.get(), sizeof ctl, hipMemcpyDeviceToHost));
            *timed_out = (int32_t) ctl[0];
        }
    }
    return VVHIP_OK;
}
int vvhip_mailbox_layout(vvhip_plan* p, int32_t* shared_device, int32_t* arithmetic_layout) {
    NEED_BOUND(p);
    if (shared_device) *shared_device = p->mb_shared_device ? 1 : 0;
    if (arithmetic_layout) *arithmetic_layout = (use_mailbox(p) && periodic_b(p)) ? 1 : 0;
    return VVHIP_OK;
}
int vvhip_mailbox_destroy(vvhip_plan* p) {
    NEED_BOUND(p);
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    drop_graphs(p);
    mailbox_release(p);
    return VVHIP_OK;
}

int vvhip_comm_destroy(vvhip_plan* p) {
    if (!p) return VVHIP_ERR_INVALID;
    if (p->comm) { (void) hipStreamSynchronize(p->stream); (void) rccl_api().commDestroy(p->comm); p->comm = nullptr; p->comm_ranks = 1; }
    return VVHIP_OK;
}

}  // extern "C"
