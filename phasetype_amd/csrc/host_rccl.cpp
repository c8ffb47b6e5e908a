/*
 * host_rccl.cpp — RCCL bound at run time (RcclApi, host_internal.h) and the
 * entry points that attach a communicator to a context.
 */
#include <dlfcn.h>

#include "host_internal.h"

using namespace pht;
using namespace pht::host;

RcclApi &pht::host::rccl() {
  static RcclApi a;
  static std::once_flag once;
  std::call_once(once, [] {
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return;
    a.getUniqueId = (decltype(a.getUniqueId))dlsym(h, "ncclGetUniqueId");
    a.commInitRank = (decltype(a.commInitRank))dlsym(h, "ncclCommInitRank");
    a.allReduce = (decltype(a.allReduce))dlsym(h, "ncclAllReduce");
    a.commDestroy = (decltype(a.commDestroy))dlsym(h, "ncclCommDestroy");
    a.errStr = (decltype(a.errStr))dlsym(h, "ncclGetErrorString");
    a.ok = a.getUniqueId && a.commInitRank && a.allReduce && a.commDestroy && a.errStr;
  });
  return a;
}

extern "C" int pht_rccl_unique_id(unsigned char *id) {
  if (!id) {
    set_err("pht_rccl_unique_id: null buffer");
    return -1;
  }
  if (!rccl().ok) {
    set_err("RCCL (librccl.so.1) could not be loaded");
    return -1;
  }
  ncclUniqueId u;
  const ncclResult_t r = rccl().getUniqueId(&u);
  if (r != ncclSuccess) {
    set_err("ncclGetUniqueId failed: %s", rccl().errStr(r));
    return -1;
  }
  memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
  return 0;
}

/* Every local precondition of pht_ctx_attach_rccl and pht_ctx_rccl_allreduce,
 * checked BEFORE any rank enters a collective: RCCL loadable, no communicator
 * attached yet, the device selectable, and the staging buffer of the
 * all-reduce self-test (max_len int64 words) allocated.  The caller agrees on
 * the verdict across ranks first (phasetype_amd/dist.py attach_rccl), so a
 * rank that fails here cannot leave its peers waiting in ncclCommInitRank. */
extern "C" int pht_ctx_rccl_prepare(pht_ctx *c, int max_len) {
  if (!c || max_len < 1) {
    set_err("pht_ctx_rccl_prepare: need a context and max_len >= 1");
    return -1;
  }
  if (c->comm) {
    set_err("pht_ctx_rccl_prepare: a communicator is already attached");
    return -1;
  }
  if (!rccl().ok) {
    set_err("RCCL (librccl.so.1) could not be loaded");
    return -1;
  }
  if (hipSetDevice(c->device) != hipSuccess) {
    set_err("pht_ctx_rccl_prepare: device %d", c->device);
    return -1;
  }
  if (c->d_rccl && c->rccl_cap < max_len) {
    c->d_rccl.reset();
    c->rccl_cap = 0;
  }
  if (!c->d_rccl && c->d_rccl.alloc(max_len) != hipSuccess) {
    set_err("pht_ctx_rccl_prepare: no device memory for %d words", max_len);
    return -1;
  }
  /* the agreed word count of every later pht_ctx_rccl_allreduce (ranks
   * prepare with the same max_len; a larger buffer kept from before is
   * reduced only over these words) */
  c->rccl_cap = max_len;
  return 0;
}

/* The collective step only: ncclCommInitRank with the broadcast id.  Needs
 * pht_ctx_rccl_prepare first (agreed across ranks). */
extern "C" int pht_ctx_attach_rccl(pht_ctx *c, const unsigned char *id, int nranks, int rank) {
  if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) {
    set_err("pht_ctx_attach_rccl: need a context, a unique id and 0 <= rank < nranks");
    return -1;
  }
  if (c->comm || !c->d_rccl || !rccl().ok) {
    set_err("pht_ctx_attach_rccl: call pht_ctx_rccl_prepare first (and agree on it across ranks)");
    return -1;
  }
  (void)hipSetDevice(c->device);
  ncclUniqueId u;
  memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
  ncclComm_t comm = nullptr;
  const ncclResult_t r = rccl().commInitRank(&comm, nranks, u, rank);
  if (r != ncclSuccess) {
    set_err("ncclCommInitRank (rank %d of %d) failed: %s", rank, nranks, rccl().errStr(r));
    return -1;
  }
  c->comm = comm;
  return 0;
}

/* in-place sum of a host int64 vector over the context's communicator, on its
 * stream (the same all-reduce a sweep runs on its statistics block): the
 * attach-time self-test of phasetype_amd/dist.py compares it with
 * torch.distributed's sum.  The staging buffer comes from
 * pht_ctx_rccl_prepare; once the communicator exists this rank always enters
 * the all-reduce, even when its upload failed (the error is reported after
 * the collective), so its peers are never left waiting. */
extern "C" int pht_ctx_rccl_allreduce(pht_ctx *c, long long *buf, int len) {
  if (!c || !c->comm) {
    set_err("pht_ctx_rccl_allreduce: need a context with an RCCL communicator");
    return -1;
  }
  /* every rank reduces exactly the prepared word count (the same on every
   * rank, pht_ctx_rccl_prepare), whatever len it was given: a bad length on
   * one rank alone then still matches its peers' collective (its words are
   * zeros), and the error is reported afterwards */
  const bool badlen = !buf || len < 1 || len > c->rccl_cap;
  const int nred = c->rccl_cap;
  (void)hipSetDevice(c->device);
  long long *d = c->d_rccl.get();
  hipStream_t st = c->stream.get();
  hipError_t e = hipMemsetAsync(d, 0, sizeof(long long) * nred, st);
  if (e == hipSuccess && !badlen) e = hipMemcpyAsync(d, buf, sizeof(long long) * len, hipMemcpyHostToDevice, st);
  const ncclResult_t r = rccl().allReduce(d, d, (size_t)nred, ncclUint64, ncclSum, c->comm, st);
  if (e == hipSuccess && r == ncclSuccess && !badlen)
    e = hipMemcpyAsync(buf, d, sizeof(long long) * len, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (badlen) {
    set_err("pht_ctx_rccl_allreduce: need 1 <= len <= the prepared size (%d), got %d", c->rccl_cap, len);
    return -1;
  }
  if (r != ncclSuccess) {
    set_err("RCCL all-reduce failed: %s", rccl().errStr(r));
    return -1;
  }
  if (e != hipSuccess) {
    set_err("pht_ctx_rccl_allreduce: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}
