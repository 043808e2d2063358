/* fd_verify_svc.hip -- the per-GPU verify service (include/fd_verify_svc.h):
   the GPU tile's side of the shared-memory protocol.

   One process per GPU owns the HIP context.  Every verify tile it serves
   posts requests (a seq range of an unpolled quic_verify link, or frags it
   copied from a polled link) into its slots of the segment.  The service
   copies each newly posted request's frags into HBM at once, then merges
   the ingested requests of all tiles into one verify launch (up to
   batch_max frags), so a launch is C4-sized whatever the tile count:

     k_svc_gather   (the ingest: the newly posted requests of every tile in
                    one launch on the ingest stream, as soon as they are
                    posted) one wave per frag: before_frag's share (range
                    requests name only the kept seqs: seq0 + i x rr_cnt),
                    the mcache line (seq still there, chunk in [chunk0,
                    wmark], sz <= FD_TPU_RAW_MTU: fd_stem.c and during_frag's
                    checks, fd_verify_tile.c:74-76), and the frag's bytes
                    from the link's dcache (pinned host memory) into the
                    request slot's HBM ingest frags.  Then the kernel's last
                    workgroup puts the slot to INGESTED: the tile checks
                    for overruns and returns the link's credits right away,
                    so the link holds a frag for the PCIe copy only, not for
                    the merge and the verify
     k_svc_assemble the verify launch's per-frag arrays from its requests'
                    ingest frags
     fd_txn_hip_batch_core
                    k_txnm_batch<16> (during_frag's copy into the request's
                    HBM staging frags, fd_txn_parse, the sig0 tag with each
                    tile's seed, the signature records), the verify, the
                    per-txn fd_ed25519_verify_batch_single_msg reduce
     k_svc_results  32-B result records, written straight into each
                    request slot's result array in the segment (registered
                    host memory); then the slot goes to RESULTS

   The out frags stay in HBM.  After its ordered pass (tcache, bundles) the
   tile posts flushes: out entries (frag, chunk, realized size) of the frags
   it publishes, chunks assigned as after_frag assigns them.  The newly
   posted flushes of every tile go into one flush batch: one kernel
   (k_svc_compact) on the flush stream that writes those staging frags
   straight into each tile's out dcache (registered host memory) at their
   chunks: whole 64-B chunks in 16-B stores, each frag contiguous, so the
   PCIe writes are full lines.  Only published frags cross PCIe.

   Host work per step is a few HIP calls: descriptors live in mapped pinned
   memory the kernels read in place, and results and flushed frags are
   written by kernels, not copied -- no hipMemcpy on the steady-state path.
   A flush batch costs one launch and one event, an ingest one launch and
   two events, a verify launch its kernels and two events.  The service
   thread drives the verify launches and the flushes; the ingest side
   (retiring gathers, starting new ones) runs on a thread of its own when
   the process may run on two CPUs or more, else inside the service
   thread's poll.

   Three kinds of stream: the ingest stream (gathers, in order), the flush
   stream (flush batches, retired in order, each flush advancing its tile's
   flush_done, so a tile's flushes finish in the order it posted them) and
   one stream per verify launch in flight.  Every HIP failure aborts (the
   reference's FD_LOG_ERR ends a tile; a device error is never turned into
   a verdict).

   Round 6 built and measured other forms of the ingest and flush side (a
   persistent kernel polling the rings, a quarter wave per frag, one flush
   stream per tile, a second ingest stream, stream priorities, CU-masked
   verify streams); each lost its A/B and is gone (DESIGN.md section 11
   has the measurements and the last commit that had them). */

#include "../../include/fd_verify_svc.h"
#include "../../include/fd_verify_hip.h"
#include "fd_txn_hip_int.h"

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <pthread.h>
#include <sched.h>

#define SV_CHECK( x ) do {                                                            \
    hipError_t e_ = (x);                                                               \
    if( e_ != hipSuccess ) {                                                           \
      fprintf( stderr, "fd_verify_svc: %s failed at %s:%d: %s\n", #x, __FILE__,      \
               __LINE__, hipGetErrorString( e_ ) );                                    \
      abort();                                                                         \
    }                                                                                  \
  } while( 0 )

typedef uint8_t  u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;

#define SVC_INGEST_CHUNKS 32ul   /* an ingest frag: 2048 B (a gossip message's bound, the RAW_MTU's 1312 below it) */
#define SVC_REQ_MAX       512u   /* requests per launch (small requests at shallow link depths: 512 x 1 K frags) */
#define SVC_LAUNCH_MAX    8ul
#define SVC_GATHER_WGS    256ul  /* the gather's default grid: 1024 waves, enough to keep PCIe busy (64: 2x slower) */
#define SVC_FLUSH_WGS     256ul  /* the flush kernel's default grid */
#define SVC_REGION_MAX    64ul
#define SVC_ING_MAX       8ul    /* ingest batches in flight */
#define SVC_FB_MAX        8ul    /* flush batches in flight */
#define SVC_FB_FLUSH_MAX  512u   /* flushes per flush batch */
#define SVC_DSM_RESERVE   128ul  /* DSM workgroup slots left free in the service's verify contexts */

/* the device current on the calling thread (the service runs on one
   thread; hipSetDevice only when it changes) */
static __thread int svc_cur_dev = -1;
static void svc_device( int dev ) {
  if( svc_cur_dev != dev ) { SV_CHECK( hipSetDevice( dev ) ); svc_cur_dev = dev; }
}

static long svc_now_ns( void ) {
  struct timespec ts;
  clock_gettime( CLOCK_MONOTONIC, &ts );
  return (long)ts.tv_sec * 1000000000L + (long)ts.tv_nsec;
}

/* one request of a launch, as the gather kernel reads it (128 B) */
struct __attribute__((aligned(16))) svc_desc {
  u64 base;        /* the request's first frag in the launch */
  u64 n;
  u64 kind;        /* FD_VERIFY_SVC_REQ_* */
  u64 src;         /* RANGE: the mcache's line 0; FRAGS: the frag area (device addresses) */
  u64 aux0;        /* RANGE: the link's chunk base; FRAGS: the sizes */
  u64 aux1;        /* FRAGS: the kinds */
  u64 first;       /* RANGE: the first kept seq */
  u64 stride;      /* RANGE: rr_cnt */
  u64 line_mask;   /* RANGE: depth - 1 */
  u64 chunk0, wmark;
  u64 seed;
  u64 stage0;      /* staging chunk of the request's frag 0 */
  u64 ibase;       /* ingest frag of the request's frag 0 (slot (t, s): (t x req_depth + s) x slot_cap) */
  u64 res;         /* the slot's result array in the segment (device address; verify launches) */
  u64 state;       /* the request slot's state word in the segment (device address; ingests: the kernel's last
                      workgroup stores INGESTED there itself) */
};
static_assert( sizeof(svc_desc) == 128, "svc_desc layout" );

/**********************************************************************/
/* kernels                                                             */

typedef u32 v4u __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) v4u gv4u;     /* global memory: global_load / global_store, not flat */

/* the ingest: one wave per frag, descriptors read in place from mapped
   host memory */
__global__ __launch_bounds__(256)
void k_svc_gather( svc_desc const * __restrict__ desc, u32 nreq, ulong n, u8 * __restrict__ ing,
                   u16 * __restrict__ ing_sz, u8 * __restrict__ ing_kind, u32 * __restrict__ ing_tso,
                   u8 * __restrict__ stage, u32 * __restrict__ done_ctr ) {
  __shared__ u64 sbase[SVC_REQ_MAX];
  for( u32 i = threadIdx.x; i < nreq; i += blockDim.x ) sbase[i] = desc[i].base;
  __syncthreads();
  u32 const lane = threadIdx.x & 63u;
  /* one wave per frag, grid-stride: a grid of n/4 workgroups takes each frag
     once; a capped grid (gather_wgs) loops */
  for( ulong j = (ulong)blockIdx.x * 4ul + (threadIdx.x >> 6); j < n; j += 4ul * gridDim.x ) {
    u32 lo = 0u, hi = nreq;                                 /* sbase[lo] <= j < sbase[hi] */
    while( hi - lo > 1u ) { u32 mid = (lo + hi) >> 1; if( sbase[mid] <= j ) lo = mid; else hi = mid; }
    svc_desc const * d = desc + lo;
    ulong const i = j - d->base;
    u32 sz = 0u, kind = FD_VERIFY_HIP_IN_QUIC, tsv = 0u;
    bool ok;
    u8 const * src;
    if( d->kind == FD_VERIFY_SVC_REQ_RANGE ) {
      ulong const seq = d->first + i * d->stride;
      u8 const * line = (u8 const *)d->src + 32ul * (seq & d->line_mask);
      /* lanes 0 and 1 read the line's two halves (seq, sig | chunk, sz,
         ctl, tsorig, tspub) with vector loads, every lane takes them */
      uint4 v = make_uint4( 0u, 0u, 0u, 0u );
      if( lane < 2u ) v = *(uint4 const *)(line + 16u * lane);
      u64 const found = (u64)(u32)__shfl( (int)v.x, 0 ) | ((u64)(u32)__shfl( (int)v.y, 0 ) << 32);
      u32 const chunk = (u32)__shfl( (int)v.x, 1 );
      sz  = (u32)__shfl( (int)v.y, 1 ) & 0xffffu;
      tsv = (u32)__shfl( (int)v.z, 1 );
      ok  = found == seq && (ulong)chunk >= d->chunk0 && (ulong)chunk <= d->wmark && sz <= FD_VERIFY_HIP_TPU_RAW_MTU;
      src = (u8 const *)d->aux0 + 64ul * chunk;
    } else {
      src  = (u8 const *)d->src + FD_VERIFY_SVC_FRAG_STRIDE * i;
      sz   = ((u16 const *)d->aux0)[i];
      bool const sigs = d->kind == FD_VERIFY_SVC_REQ_SIGS;   /* a client's signature records: no frag kind */
      kind = sigs ? FD_VERIFY_HIP_IN_QUIC : ((u8 const *)d->aux1)[i];
      ok   = sz <= FD_VERIFY_SVC_FRAG_STRIDE && ( !sigs || sz >= FD_VERIFY_SVC_SIG_HDR_SZ );
    }
    ulong const f = d->ibase + i;
    u8 * dst = ing + 64ul * SVC_INGEST_CHUNKS * f;
    if( ok ) for( u32 p = 16u * lane; p < sz; p += 1024u ) *(uint4 *)(dst + p) = *(uint4 const *)(src + p);
    /* a gossip vote's out header: the reference writes four fields into the
       out chunk's stale header (fd_verify_tile.c:90-93); here the rest is 0 */
    if( kind == FD_VERIFY_HIP_IN_GOSSIP && lane < 5u )
      *(uint4 *)(stage + 64ul * (d->stage0 + FD_TXN_HIP_STAGE_CHUNKS * i) + 16u * lane) = make_uint4( 0u, 0u, 0u, 0u );
    if( lane == 0u ) { ing_sz[f] = ok ? (u16)sz : (u16)0xffffu; ing_kind[f] = (u8)kind; ing_tso[f] = tsv; }
  }
  /* INGESTED from the GPU: once every workgroup has passed its loop (all of
     its loads from the links have returned), the last one stores INGESTED
     into each request's slot in the segment, so a tile may reuse its link
     without waiting for the service thread's turn (the service still
     retires the batch by its event before a verify launch reads the HBM
     frags).  done_ctr: this batch's counter, zero at launch; the last
     workgroup puts it back to zero for the next batch on the ingest stream */
  /* Only the links' reads must be over (their values were stored, so they
     have returned): no fence, and relaxed stores -- a system-scope release
     here would write the whole L2 back (the verify kernels' dirty lines
     included) once per request, which measured slower than the host's
     turn it saves */
  if( !done_ctr ) return;
  __syncthreads();
  __shared__ u32 last;
  if( threadIdx.x == 0u ) last = atomicAdd( done_ctr, 1u ) == gridDim.x - 1u;
  __syncthreads();
  if( !last ) return;
  for( u32 i = threadIdx.x; i < nreq; i += blockDim.x )
    if( desc[i].state )
      __hip_atomic_store( (u64 *)desc[i].state, (u64)FD_VERIFY_SVC_INGESTED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
  if( threadIdx.x == 0u ) *done_ctr = 0u;
}

/* a verify launch's per-frag arrays (launch frag j = frag i of request d)
   from the requests' ingest frags: one thread per frag */
__global__ __launch_bounds__(256)
void k_svc_assemble( svc_desc const * __restrict__ desc, u32 nreq, ulong n, u16 const * __restrict__ ing_sz,
                     u8 const * __restrict__ ing_kind, u32 const * __restrict__ ing_tso, u32 * __restrict__ in_chunk,
                     u16 * __restrict__ in_sz, u8 * __restrict__ in_kind, u32 * __restrict__ tso, u64 * __restrict__ seedv,
                     u32 * __restrict__ stage_chunk ) {
  __shared__ u64 sbase[SVC_REQ_MAX];
  for( u32 i = threadIdx.x; i < nreq; i += blockDim.x ) sbase[i] = desc[i].base;
  __syncthreads();
  ulong const j = (ulong)blockIdx.x * blockDim.x + threadIdx.x;
  if( j >= n ) return;
  u32 lo = 0u, hi = nreq;
  while( hi - lo > 1u ) { u32 mid = (lo + hi) >> 1; if( sbase[mid] <= j ) lo = mid; else hi = mid; }
  svc_desc const * d = desc + lo;
  ulong const i = j - d->base, f = d->ibase + i;
  in_chunk[j] = (u32)(SVC_INGEST_CHUNKS * f); in_sz[j] = ing_sz[f]; in_kind[j] = ing_kind[f]; tso[j] = ing_tso[f];
  seedv[j] = d->seed; stage_chunk[j] = (u32)(d->stage0 + FD_TXN_HIP_STAGE_CHUNKS * i);
}

__global__ __launch_bounds__(256)
void k_svc_results( svc_desc const * __restrict__ desc, u32 nreq, ulong n, u16 const * __restrict__ tsz,
                    u64 const * __restrict__ tag, u64 const * __restrict__ bid, u8 const * __restrict__ cnt,
                    signed char const * __restrict__ tcode, u64 const * __restrict__ fdesc, u32 const * __restrict__ tso ) {
  __shared__ u64 sbase[SVC_REQ_MAX];
  for( u32 i = threadIdx.x; i < nreq; i += blockDim.x ) sbase[i] = desc[i].base;
  __syncthreads();
  ulong const j = (ulong)blockIdx.x * blockDim.x + threadIdx.x;
  if( j >= n ) return;
  u32 lo = 0u, hi = nreq;
  while( hi - lo > 1u ) { u32 mid = (lo + hi) >> 1; if( sbase[mid] <= j ) lo = mid; else hi = mid; }
  u64 const d = fdesc[j];
  u32 const cend = (u32)(d & 0xfffu), psz = (u32)((d >> 12) & 0x7ffu);
  bool const gossip = (d >> 33) & 1u, bad = (d >> 34) & 1u;
  fd_verify_svc_res_t r;
  r.tag = tag[j]; r.bundle_id = bid[j]; r.txn_t_sz = tsz[j]; r.payload_sz = (u16)psz; r.code = tcode[j];
  r.flags = bad ? (u8)FD_VERIFY_SVC_RES_BAD
                : (!gossip && cend < FD_VERIFY_HIP_TXNM_SZ + psz) ? (u8)FD_VERIFY_SVC_RES_HOST : (u8)0;
  r.sig_cnt = cnt[j]; r.rsv0 = 0u; r.tsorig = tso[j]; r.rsv1 = 0u;
  /* straight into the slot's result array in the (registered) segment: a
     wave writes 2 KB contiguous */
  ((fd_verify_svc_res_t *)desc[lo].res)[j - sbase[lo]] = r;
}

/* a signature launch (FD_VERIFY_SVC_REQ_SIGS, include/fd_verify_svc.h
   "clients"): record j of the launch (record i of request d) from its
   ingest frag -- signature, public key, message -- into the verify's
   inputs: the signature and key into the launch's record arrays, the
   message into the request slot's staging frag i (a client's slots are
   never flushed; staging offsets fit the verify's 32-bit msg_off).  One
   wave per record, grid-stride. */
__global__ __launch_bounds__(256)
void k_svc_sigrec( svc_desc const * __restrict__ desc, u32 nreq, ulong n, u8 const * __restrict__ ing,
                   u16 const * __restrict__ ing_sz, u8 * __restrict__ stage, u8 * __restrict__ rsig,
                   u8 * __restrict__ rpub, u32 * __restrict__ rmoff, u32 * __restrict__ rmsz ) {
  __shared__ u64 sbase[SVC_REQ_MAX];
  for( u32 i = threadIdx.x; i < nreq; i += blockDim.x ) sbase[i] = desc[i].base;
  __syncthreads();
  u32 const lane = threadIdx.x & 63u;
  for( ulong j = (ulong)blockIdx.x * 4ul + (threadIdx.x >> 6); j < n; j += 4ul * gridDim.x ) {
    u32 lo = 0u, hi = nreq;
    while( hi - lo > 1u ) { u32 mid = (lo + hi) >> 1; if( sbase[mid] <= j ) lo = mid; else hi = mid; }
    svc_desc const * d = desc + lo;
    ulong const i = j - d->base, f = d->ibase + i;
    u32 const sz = ing_sz[f];
    bool const ok = sz != 0xffffu;                             /* the gather checked 96 <= sz <= the stride */
    u32 const msz = ok ? sz - (u32)FD_VERIFY_SVC_SIG_HDR_SZ : 0u;
    u8 const * src = ing + 64ul * SVC_INGEST_CHUNKS * f;
    ulong const moff = 64ul * (d->stage0 + FD_TXN_HIP_STAGE_CHUNKS * i);
    if( lane < 4u )      *(uint4 *)(rsig + 64ul * j + 16u * lane) = ok ? *(uint4 const *)(src + 16u * lane) : make_uint4( 0u, 0u, 0u, 0u );
    else if( lane < 6u ) *(uint4 *)(rpub + 32ul * j + 16u * (lane - 4u)) = ok ? *(uint4 const *)(src + 16u * lane) : make_uint4( 0u, 0u, 0u, 0u );
    /* the message: 16-B pieces from ingest byte 96 on (both 16-B aligned) */
    for( u32 p = 16u * lane; p < msz; p += 1024u )
      *(uint4 *)(stage + moff + p) = *(uint4 const *)(src + FD_VERIFY_SVC_SIG_HDR_SZ + p);
    if( lane == 0u ) { rmoff[j] = (u32)moff; rmsz[j] = msz; }
  }
}

/* a signature launch's results into the requests' result arrays */
__global__ __launch_bounds__(256)
void k_svc_sigres( svc_desc const * __restrict__ desc, u32 nreq, ulong n, u16 const * __restrict__ ing_sz,
                   signed char const * __restrict__ rcode ) {
  __shared__ u64 sbase[SVC_REQ_MAX];
  for( u32 i = threadIdx.x; i < nreq; i += blockDim.x ) sbase[i] = desc[i].base;
  __syncthreads();
  ulong const j = (ulong)blockIdx.x * blockDim.x + threadIdx.x;
  if( j >= n ) return;
  u32 lo = 0u, hi = nreq;
  while( hi - lo > 1u ) { u32 mid = (lo + hi) >> 1; if( sbase[mid] <= j ) lo = mid; else hi = mid; }
  svc_desc const * d = desc + lo;
  u32 const sz = ing_sz[d->ibase + (j - sbase[lo])];
  bool const ok = sz != 0xffffu;
  fd_verify_svc_res_t r;
  r.tag = 0ul; r.bundle_id = 0ul; r.txn_t_sz = 0u; r.payload_sz = ok ? (u16)(sz - FD_VERIFY_SVC_SIG_HDR_SZ) : (u16)0;
  r.code = ok ? rcode[j] : (signed char)-1;                     /* FD_ED25519_ERR_SIG */
  r.flags = ok ? (u8)0 : (u8)FD_VERIFY_SVC_RES_BAD;
  r.sig_cnt = ok ? (u8)1 : (u8)0; r.rsv0 = 0u; r.tsorig = 0u; r.rsv1 = 0u;
  ((fd_verify_svc_res_t *)d->res)[j - sbase[lo]] = r;
}

/* one flush of a flush batch (64 B) */
struct __attribute__((aligned(16))) svc_fdesc {
  u64 base;        /* the flush's first entry in the batch */
  u64 out;         /* its out entries (device address) */
  u64 stage0;
  u64 dcache;      /* the tile's out dcache (device address) */
  long delta;
  u64 out_sz;
  u64 err;         /* the tile's error flag (device address) */
  u64 rsv;
};
static_assert( sizeof(svc_fdesc) == 64, "svc_fdesc layout" );

/* a flush batch: the newly posted flushes of every tile in one launch.
   Entry j of the batch is entry j - base of the flush whose range holds it;
   its staging frag (its realized bytes, in whole 64-B chunks) goes straight
   into its tile's out dcache (registered host memory) at the entry's chunk:
   one wave per entry, grid-stride (a capped grid, flush_wgs, loops), 16-B
   stores, a frag's bytes contiguous */
__global__ __launch_bounds__(256)
void k_svc_compact( svc_fdesc const * __restrict__ fd, u32 nf, ulong n, u8 const * __restrict__ stage,
                    ulong slot_cap ) {
  __shared__ u64 sbase[SVC_FB_FLUSH_MAX];
  for( u32 i = threadIdx.x; i < nf; i += blockDim.x ) sbase[i] = fd[i].base;
  __syncthreads();
  u32 const lane = threadIdx.x & 63u;
  for( ulong j = (ulong)blockIdx.x * 4ul + (threadIdx.x >> 6); j < n; j += 4ul * gridDim.x ) {
    u32 lo = 0u, hi = nf;
    while( hi - lo > 1u ) { u32 mid = (lo + hi) >> 1; if( sbase[mid] <= j ) lo = mid; else hi = mid; }
    svc_fdesc const * d = fd + lo;
    fd_verify_svc_out_t const o = ((fd_verify_svc_out_t const *)d->out)[j - sbase[lo]];
    if( o.flags & FD_VERIFY_SVC_OUT_HOSTWRITTEN ) continue;
    u32 const len = ((u32)o.sz + 63u) & ~63u;
    long const at = (long)(64ul * (ulong)o.chunk) + d->delta;
    /* the entry comes from the tile, an untrusted peer: its frag must be one
       of the slot's staging frags (idx below slot_cap, at most a staging
       frag's bytes) and its chunk must lie inside its out dcache.  A bad
       entry is reported (the service aborts at the flush's retirement),
       never read or written (an idx past the slot read other
       tiles' staging or past the allocation) */
    if( (ulong)o.idx >= slot_cap || len > 64u * (u32)FD_TXN_HIP_STAGE_CHUNKS || at < 0 || at + (long)len > (long)d->out_sz ) {
      if( lane == 0u ) *(volatile u32 *)d->err = 1u;
      continue;
    }
    u8 const * src = stage + 64ul * (d->stage0 + FD_TXN_HIP_STAGE_CHUNKS * (ulong)o.idx);
    u8 *       dst = (u8 *)d->dcache + at;
    for( u32 p = 16u * lane; p < len; p += 1024u ) *(uint4 *)(dst + p) = *(uint4 const *)(src + p);
  }
}

/**********************************************************************/
/* service                                                             */

struct svc_launch {
  int                    busy;
  int                    sig;            /* a signature launch (FD_VERIFY_SVC_REQ_SIGS requests) */
  fd_ed25519_hip_ctx_t * ctx;
  hipStream_t            st;
  hipEvent_t             ev0, ev1;
  u32 * d_in_chunk; u16 * d_in_sz; u8 * d_in_kind; u32 * d_tso; u64 * d_seed; u32 * d_stage_chunk;
  u16 * d_tsz; u64 * d_tag; u64 * d_bid; u32 * d_first; u8 * d_cnt; signed char * d_tcode; u32 * d_misc;
  u8 *  d_rsig; u8 * d_rpub; u32 * d_rmoff; u32 * d_rmsz; signed char * d_rcode; ulong rcap; u64 * d_fdesc;
  svc_desc * h_desc; svc_desc * d_desc;   /* mapped pinned memory: the kernels read h_desc at d_desc */
  ulong nreq, n;
  struct { ulong t, slot; } req[SVC_REQ_MAX];
};

struct svc_tile {
  int          set;
  int          client;         /* FD_VERIFY_SVC_REQ_SIGS only, no out dcache (fd_verify_svc_set_client) */
  u8 *         h_out;          /* the out dcache (host) */
  ulong        out_sz;
  u8 const *   chunk_base;     /* host address of out chunk 0 */
  u8 *         d_out;          /* the out dcache's device address (registered) */
  u32 *        h_err;          /* mapped pinned: a flush found an entry outside the out dcache */
  u32 *        d_err;
  ulong        take;          /* next request id to take */
  ulong        flush_take;     /* next flush to start */
  ulong        flush_fin;      /* flushes retired */
};

struct svc_pend { ulong t, slot, n; long seen; ulong sig; };

/* a flush batch: every tile's newly posted flushes (up to
   SVC_FB_FLUSH_MAX) in one k_svc_compact launch on the flush
   stream; retired in order, each flush's tile advancing flush_done */
struct svc_fbatch {
  int         busy;
  hipEvent_t  ev;
  svc_fdesc * h_desc; svc_fdesc * d_desc;   /* mapped pinned memory */
  u32         nf;
  ulong       n;
  u8          t[SVC_FB_FLUSH_MAX];          /* each flush's tile */
};

/* an ingest batch: the gather of newly posted requests, on the ingest stream */
struct svc_ingest {
  int         busy;
  hipEvent_t  ev0, ev1;
  svc_desc *  h_desc; svc_desc * d_desc;   /* mapped pinned memory */
  ulong       nreq, n;
  struct { ulong t, slot; } req[SVC_REQ_MAX];
};

struct fd_verify_svc {
  fd_verify_svc_seg_t * seg;
  int      dev;
  ulong    batch_max, inflight;
  ulong    merge_min; long merge_wait_ns;
  /* two numeric tunables (grid sizes, not paths) */
  ulong    gather_wgs;   /* the gather's grid cap (0: one wave per frag); FD_VERIFY_SVC_GATHER_WGS, default
                            SVC_GATHER_WGS: a grid of one wave per frag fills the GPU with waves that wait on
                            PCIe reads, and the verify launches beside it ran ~12% slower (profiles/r05u,v) */
  ulong    flush_wgs;    /* the flush kernel's grid cap (0: one wave per entry); FD_VERIFY_SVC_FLUSH_WGS, default
                            SVC_FLUSH_WGS (profiles/r05w: 3 tiles 65-68 vs 61-64 M uncapped) */
  struct { u8 * h; ulong sz; u8 * d; } reg[SVC_REGION_MAX];
  ulong    nreg;
  struct { int set; u8 const * d_mcache; ulong depth; u8 const * d_base; ulong chunk0, wmark; } link[FD_VERIFY_SVC_LINK_MAX];
  svc_tile tile[FD_VERIFY_SVC_TILE_MAX];
  u8 *     d_stage;            /* staging: tile x slot x slot_cap frags of FD_TXN_HIP_STAGE_CHUNKS */
  u8 *     d_ing;              /* ingest: tile x slot x slot_cap frags of SVC_INGEST_CHUNKS */
  u16 *    d_ing_sz; u8 * d_ing_kind; u32 * d_ing_tso;   /* per ingest frag */
  hipStream_t st_ing;          /* every gather, in order */
  svc_ingest ING[SVC_ING_MAX];
  ulong    ing_take, ing_fin;  /* ingest batches started / retired (ring order) */
  u32 *    d_ing_ctr;          /* per ingest batch slot: k_svc_gather's workgroups done (HBM, zero between batches) */
  hipStream_t st_flush;        /* every flush batch, in order */
  svc_fbatch FB[SVC_FB_MAX];
  ulong    fb_take, fb_fin;
  svc_desc * sdesc;            /* per (tile, slot): the request's descriptor, made at ingest */
  svc_launch L[SVC_LAUNCH_MAX];
  svc_pend * pend; ulong pend_cap, pend_head, pend_tail, pend_frags;
  svc_pend * spend; ulong spend_head, spend_tail;   /* ingested signature requests (clients), their own queue:
                                                       they ride signature launches, not the merge of txn frags */
  ulong    occ[6];             /* every 64th poll with a slot in use: samples, then the summed slot counts posted (not yet
                                  ingested), ingested and waiting for a launch, in a launch, results (the
                                  tile's ordered pass, flushes, publish), free */
  ulong    stat[16];           /* launches, frags, requests, flushes, flushed frags, flushed bytes, flush kernels, gpu ns;
                                  host ns starting launches, starting flushes, retiring, polls; ingests, ingest
                                  gpu ns, host ns starting ingests, the largest launch */
  long     merge_idle_ns;      /* a launch on an idle GPU once the oldest request has waited this long */
  int      running;
  /* the ingest side (steps 1b and 2 of the poll: retire finished gathers,
     gather newly posted requests) on a thread of its own when the process
     may run on two or more CPUs: a range request holds its link until its
     gather has read it, and on one thread a new request waited behind the
     flush and launch work of every other tile (profiles/r06/gpu_ingested:
     the service thread's ingest and flush turns filled the run).  The
     one-thread loop stays, selected from the CPU affinity: it is the only
     path on one CPU, and FD_VERIFY_SVC_INGEST_THREAD=0 forces it.  Ingested
     requests reach the launch queues through ih, a single-producer
     single-consumer ring (ih_tail: stored by the ingest side with release;
     sdesc is written before it) */
  int      ithread;            /* the ingest thread runs */
  pthread_t ith;
  int      istop;
  int      iready;             /* the ingest thread has made its first HIP calls */
  int      iexited;            /* the ingest thread has left its loop */
  svc_pend * ih; ulong ih_cap; ulong ih_tail, ih_head;
  long     launch_t0[SVC_LAUNCH_MAX];           /* a verify launch's start (the stuck-launch watchdog) */
};

static u8 * svc_dev( fd_verify_svc_t * s, void const * h, ulong sz ) {
  u8 const * p = (u8 const *)h;
  for( ulong k = 0; k < s->nreg; k++ )
    if( p >= s->reg[k].h && p + sz <= s->reg[k].h + s->reg[k].sz ) return s->reg[k].d + (p - s->reg[k].h);
  fprintf( stderr, "fd_verify_svc: %p (+%lu) is in no mapped region\n", h, sz );
  abort();
}

static ulong svc_stage0( fd_verify_svc_t const * s, ulong t, ulong slot ) {
  return (t * s->seg->req_depth + slot) * s->seg->slot_cap * FD_TXN_HIP_STAGE_CHUNKS;
}

static void launch_alloc( svc_launch & L, int dev, ulong nmax ) {
  memset( &L, 0, sizeof(L) );
  L.rcap = fd_txn_hip_record_cap( nmax );
  L.ctx  = fd_ed25519_hip_ctx_new( dev, L.rcap );
  if( !L.ctx ) { fprintf( stderr, "fd_verify_svc: context creation failed\n" ); abort(); }
  /* the verify contexts' DSM grids leave SVC_DSM_RESERVE workgroup slots
     free for the gather and flush kernels beside a DSM pass (profiles/r05an:
     3 tiles 72.1 vs 69.0 M, 2 tiles 67.6 vs 66.9 M); per context, so that no
     other context of the process inherits it.  A numeric tunable: the
     environment's value wins */
  if( !getenv( "FD_ED25519_HIP_DSM_RESERVE" ) ) (void)fd_ed25519_hip_ctx_set_dsm_reserve( L.ctx, SVC_DSM_RESERVE );
  L.st = (hipStream_t)fd_ed25519_hip_ctx_stream( L.ctx );
  SV_CHECK( hipMalloc( &L.d_in_chunk, 4ul * nmax ) ); SV_CHECK( hipMalloc( &L.d_in_sz, 2ul * nmax ) );
  SV_CHECK( hipMalloc( &L.d_in_kind, nmax ) );        SV_CHECK( hipMalloc( &L.d_tso, 4ul * nmax ) );
  SV_CHECK( hipMalloc( &L.d_seed, 8ul * nmax ) );     SV_CHECK( hipMalloc( &L.d_stage_chunk, 4ul * nmax ) );
  SV_CHECK( hipMalloc( &L.d_tsz, 2ul * nmax ) );      SV_CHECK( hipMalloc( &L.d_tag, 8ul * nmax ) );
  SV_CHECK( hipMalloc( &L.d_bid, 8ul * nmax ) );      SV_CHECK( hipMalloc( &L.d_first, 4ul * nmax ) );
  SV_CHECK( hipMalloc( &L.d_cnt, nmax ) );            SV_CHECK( hipMalloc( &L.d_tcode, nmax ) );
  SV_CHECK( hipMalloc( &L.d_misc, fd_txn_hip_misc_bytes() ) );
  SV_CHECK( hipMalloc( &L.d_rsig, 64ul * L.rcap ) );  SV_CHECK( hipMalloc( &L.d_rpub, 32ul * L.rcap ) );
  SV_CHECK( hipMalloc( &L.d_rmoff, 4ul * L.rcap ) );  SV_CHECK( hipMalloc( &L.d_rmsz, 4ul * L.rcap ) );
  SV_CHECK( hipMalloc( &L.d_rcode, L.rcap ) );        SV_CHECK( hipMalloc( &L.d_fdesc, 8ul * nmax ) );
  SV_CHECK( hipHostMalloc( &L.h_desc, sizeof(svc_desc) * SVC_REQ_MAX, hipHostMallocMapped ) );
  SV_CHECK( hipHostGetDevicePointer( (void **)&L.d_desc, L.h_desc, 0 ) );
  SV_CHECK( hipEventCreate( &L.ev0 ) ); SV_CHECK( hipEventCreate( &L.ev1 ) );
}

static void launch_free( svc_launch & L ) {
  if( !L.ctx ) return;
  (void)hipStreamSynchronize( L.st );
  (void)hipFree( L.d_in_chunk ); (void)hipFree( L.d_in_sz ); (void)hipFree( L.d_in_kind );
  (void)hipFree( L.d_tso ); (void)hipFree( L.d_seed ); (void)hipFree( L.d_stage_chunk ); (void)hipFree( L.d_tsz );
  (void)hipFree( L.d_tag ); (void)hipFree( L.d_bid ); (void)hipFree( L.d_first ); (void)hipFree( L.d_cnt );
  (void)hipFree( L.d_tcode ); (void)hipFree( L.d_misc ); (void)hipFree( L.d_rsig ); (void)hipFree( L.d_rpub );
  (void)hipFree( L.d_rmoff ); (void)hipFree( L.d_rmsz ); (void)hipFree( L.d_rcode ); (void)hipFree( L.d_fdesc );
  (void)hipHostFree( L.h_desc );
  (void)hipEventDestroy( L.ev0 ); (void)hipEventDestroy( L.ev1 );
  fd_ed25519_hip_ctx_delete( L.ctx );
  L.ctx = 0;
}

extern "C" fd_verify_svc_t *
fd_verify_svc_boot( void * seg_mem, int device, ulong batch_max, ulong inflight ) {
  fd_verify_svc_seg_t * seg = fd_verify_svc_join( seg_mem );
  static_assert( FD_TXN_HIP_STAGE_CHUNKS * 64ul == FD_VERIFY_SVC_STAGE_FRAG_SZ, "staging frag size" );
  static_assert( SVC_INGEST_CHUNKS == FD_VERIFY_SVC_INGEST_CHUNKS && SVC_LAUNCH_MAX == FD_VERIFY_SVC_INFLIGHT_MAX, "limits" );
  /* the shape checks (include/fd_verify_svc.h, the same function the
     topologies' sizing is tested against): staging messages are addressed
     by 32-bit byte offsets (the verify's msg_off), ingest frags by 32-bit
     chunk indices (the parse's in_chunk) */
  if( !seg ) return 0;
  if( !fd_verify_svc_boot_ok( seg->tile_cnt, seg->req_depth, seg->slot_cap, seg->frag_cap, batch_max, inflight ) ) {
    fprintf( stderr, "fd_verify_svc: segment shape %lu tiles x %lu slots x %lu frags (frag area %lu), batch_max %lu, "
             "%lu in flight: outside the service's limits (staging %lu B, 4 GiB at most)\n", seg->tile_cnt, seg->req_depth,
             seg->slot_cap, seg->frag_cap, batch_max, inflight,
             seg->tile_cnt * seg->req_depth * seg->slot_cap * FD_VERIFY_SVC_STAGE_FRAG_SZ );
    return 0;
  }
  ulong const stage_sz = seg->tile_cnt * seg->req_depth * seg->slot_cap * FD_TXN_HIP_STAGE_CHUNKS * 64ul;
  ulong const ing_cnt  = seg->tile_cnt * seg->req_depth * seg->slot_cap;
  SV_CHECK( hipSetDevice( device ) );
  fd_verify_svc_t * s = (fd_verify_svc_t *)calloc( 1, sizeof(fd_verify_svc_t) );
  s->seg = seg; s->dev = device; s->batch_max = batch_max; s->inflight = inflight;
  { char const * e = getenv( "FD_VERIFY_SVC_GATHER_WGS" ); s->gather_wgs = e ? strtoul( e, 0, 0 ) : SVC_GATHER_WGS; }
  { char const * e = getenv( "FD_VERIFY_SVC_FLUSH_WGS" );  s->flush_wgs  = e ? strtoul( e, 0, 0 ) : SVC_FLUSH_WGS; }
  s->merge_min = batch_max / 2ul; s->merge_wait_ns = 2000000L; s->merge_idle_ns = 20000L;
  SV_CHECK( hipMalloc( &s->d_stage, stage_sz + 4096ul ) );
  SV_CHECK( hipMalloc( &s->d_ing, 64ul * SVC_INGEST_CHUNKS * ing_cnt + 4096ul ) );
  SV_CHECK( hipMalloc( &s->d_ing_sz, 2ul * ing_cnt ) ); SV_CHECK( hipMalloc( &s->d_ing_kind, ing_cnt ) );
  SV_CHECK( hipMalloc( &s->d_ing_tso, 4ul * ing_cnt ) );
  SV_CHECK( hipMalloc( &s->d_ing_ctr, 4ul * SVC_ING_MAX ) ); SV_CHECK( hipMemset( s->d_ing_ctr, 0, 4ul * SVC_ING_MAX ) );
  /* the ingest and flush streams, at the default priority (the greatest
     lost its A/B, profiles/r06/io_prio) */
  SV_CHECK( hipStreamCreateWithPriority( &s->st_ing, hipStreamNonBlocking, 0 ) );
  for( ulong k = 0; k < SVC_ING_MAX; k++ ) {
    svc_ingest & I = s->ING[k];
    SV_CHECK( hipHostMalloc( &I.h_desc, sizeof(svc_desc) * SVC_REQ_MAX, hipHostMallocMapped ) );
    SV_CHECK( hipHostGetDevicePointer( (void **)&I.d_desc, I.h_desc, 0 ) );
    SV_CHECK( hipEventCreate( &I.ev0 ) ); SV_CHECK( hipEventCreate( &I.ev1 ) );
  }
  SV_CHECK( hipStreamCreateWithPriority( &s->st_flush, hipStreamNonBlocking, 0 ) );
  for( ulong k = 0; k < SVC_FB_MAX; k++ ) {
    svc_fbatch & F = s->FB[k];
    SV_CHECK( hipHostMalloc( &F.h_desc, sizeof(svc_fdesc) * SVC_FB_FLUSH_MAX, hipHostMallocMapped ) );
    SV_CHECK( hipHostGetDevicePointer( (void **)&F.d_desc, F.h_desc, 0 ) );
    SV_CHECK( hipEventCreateWithFlags( &F.ev, hipEventDisableTiming ) );
  }
  s->sdesc = (svc_desc *)calloc( seg->tile_cnt * seg->req_depth, sizeof(svc_desc) );
  for( ulong k = 0; k < inflight; k++ ) launch_alloc( s->L[k], device, batch_max );
  s->pend_cap = seg->tile_cnt * seg->req_depth;
  s->pend = (svc_pend *)calloc( s->pend_cap, sizeof(svc_pend) );
  s->spend = (svc_pend *)calloc( s->pend_cap, sizeof(svc_pend) );
  s->ih_cap = s->pend_cap;                          /* a slot's request is in the handoff ring at most once */
  s->ih = (svc_pend *)calloc( s->ih_cap, sizeof(svc_pend) );
  SV_CHECK( hipDeviceSynchronize() );
  return s;
}

extern "C" int
fd_verify_svc_map( fd_verify_svc_t * s, void * host, ulong sz ) {
  if( !s || !host || !sz || s->nreg >= SVC_REGION_MAX ) return -1;
  ulong a = (ulong)host & ~4095ul, e = ((ulong)host + sz + 4095ul) & ~4095ul;
  SV_CHECK( hipSetDevice( s->dev ) );
  if( hipHostRegister( (void *)a, e - a, hipHostRegisterMapped | hipHostRegisterPortable ) != hipSuccess ) return -1;
  void * d = 0;
  SV_CHECK( hipHostGetDevicePointer( &d, (void *)a, 0 ) );
  s->reg[s->nreg].h = (u8 *)a; s->reg[s->nreg].sz = e - a; s->reg[s->nreg].d = (u8 *)d;
  s->nreg++;
  return 0;
}

extern "C" int
fd_verify_svc_set_link( fd_verify_svc_t * s, ulong link, void const * mcache, ulong depth, void const * chunk_base,
                        ulong chunk0, ulong wmark ) {
  if( !s || link >= FD_VERIFY_SVC_LINK_MAX || !mcache || !depth || (depth & (depth - 1ul)) || chunk0 > wmark ||
      wmark > 0xffffffffull ) return -1;
  s->link[link].d_mcache = svc_dev( s, mcache, 32ul * depth );
  s->link[link].depth    = depth;
  s->link[link].d_base   = svc_dev( s, (u8 const *)chunk_base + 64ul * chunk0, 64ul * (wmark - chunk0) + 2048ul ) -
                           64ul * chunk0;
  s->link[link].chunk0   = chunk0; s->link[link].wmark = wmark;
  s->link[link].set      = 1;
  return 0;
}

extern "C" int
fd_verify_svc_set_tile( fd_verify_svc_t * s, ulong t, void * out_dcache, ulong out_sz, void const * chunk_base ) {
  if( !s || t >= s->seg->tile_cnt || !out_dcache || !out_sz || s->tile[t].set ) return -1;
  svc_tile & T = s->tile[t];
  T.d_out = svc_dev( s, out_dcache, out_sz );               /* mapped: the flush kernel writes it */
  SV_CHECK( hipHostMalloc( &T.h_err, 64, hipHostMallocMapped ) );
  SV_CHECK( hipHostGetDevicePointer( (void **)&T.d_err, T.h_err, 0 ) );
  *T.h_err = 0u;
  (void)svc_dev( s, fd_verify_svc_tile( s->seg, t ), s->seg->tile_sz );   /* the tile's part of the segment */
  SV_CHECK( hipSetDevice( s->dev ) );
  T.h_out = (u8 *)out_dcache; T.out_sz = out_sz; T.chunk_base = (u8 const *)chunk_base;
  T.set = 1;
  return 0;
}

extern "C" int
fd_verify_svc_set_client( fd_verify_svc_t * s, ulong t ) {
  if( !s || t >= s->seg->tile_cnt || s->tile[t].set ) return -1;
  (void)svc_dev( s, fd_verify_svc_tile( s->seg, t ), s->seg->tile_sz );   /* the client's part of the segment is mapped */
  s->tile[t].client = 1;
  s->tile[t].set    = 1;
  return 0;
}

extern "C" void
fd_verify_svc_set_merge( fd_verify_svc_t * s, ulong min_frags, ulong wait_ns, ulong idle_ns ) {
  s->merge_min = min_frags; s->merge_wait_ns = (long)wait_ns; s->merge_idle_ns = (long)idle_ns;
}

static void * svc_ingest_main( void * arg );

extern "C" int
fd_verify_svc_run( fd_verify_svc_t * s ) {
  for( ulong t = 0; t < s->seg->tile_cnt; t++ ) if( !s->tile[t].set ) return -1;
  svc_device( s->dev );
  /* the signature path (k_svc_sigrec, the verify's latency and bulk
     kernels, k_svc_sigres) once on zeroed records: its code objects load
     here, before the GPU tile's sandbox */
  for( ulong k = 0; k < s->inflight; k++ ) {
    svc_launch & L = s->L[k];
    SV_CHECK( hipMemsetAsync( L.d_rsig, 0, 64ul * 256ul, L.st ) ); SV_CHECK( hipMemsetAsync( L.d_rpub, 0, 32ul * 256ul, L.st ) );
    SV_CHECK( hipMemsetAsync( L.d_rmoff, 0, 4ul * 256ul, L.st ) ); SV_CHECK( hipMemsetAsync( L.d_rmsz, 0, 4ul * 256ul, L.st ) );
    hipLaunchKernelGGL( k_svc_sigrec, dim3( 1 ), dim3( 256 ), 0, L.st, L.d_desc, 0u, 0ul, (u8 const *)s->d_ing,
                        (u16 const *)s->d_ing_sz, s->d_stage, L.d_rsig, L.d_rpub, L.d_rmoff, L.d_rmsz );
    hipLaunchKernelGGL( k_svc_sigres, dim3( 1 ), dim3( 256 ), 0, L.st, L.d_desc, 0u, 0ul, (u16 const *)s->d_ing_sz,
                        (signed char const *)L.d_rcode );
    SV_CHECK( hipGetLastError() );
    if( fd_ed25519_hip_verify_dev( L.ctx, 1ul, L.d_rsig, L.d_rpub, s->d_stage, L.d_rmoff, L.d_rmsz, L.d_rcode, 0, L.st ) ||
        fd_ed25519_hip_verify_dev( L.ctx, 256ul, L.d_rsig, L.d_rpub, s->d_stage, L.d_rmoff, L.d_rmsz, L.d_rcode, 0, L.st ) ) {
      fprintf( stderr, "fd_verify_svc: signature path warm-up failed\n" );
      return -1;
    }
  }
  /* the kernels' code objects loaded and every buffer touched once before
     the first request (the steady state loads nothing) */
  for( ulong k = 0; k < s->inflight; k++ ) {
    svc_launch & L = s->L[k];
    hipLaunchKernelGGL( k_svc_assemble, dim3( 1 ), dim3( 256 ), 0, L.st, L.d_desc, 0u, 0ul, s->d_ing_sz, s->d_ing_kind,
                        s->d_ing_tso, L.d_in_chunk, L.d_in_sz, L.d_in_kind, L.d_tso, L.d_seed, L.d_stage_chunk );
    hipLaunchKernelGGL( k_svc_results, dim3( 1 ), dim3( 256 ), 0, L.st, L.d_desc, 0u, 0ul, L.d_tsz, L.d_tag, L.d_bid,
                        L.d_cnt, L.d_tcode, L.d_fdesc, L.d_tso );
    SV_CHECK( hipGetLastError() );
  }
  hipLaunchKernelGGL( k_svc_gather, dim3( 1 ), dim3( 256 ), 0, s->st_ing, s->ING[0].d_desc, 0u, 0ul, s->d_ing, s->d_ing_sz,
                      s->d_ing_kind, s->d_ing_tso, s->d_stage, (u32 *)0 );
  SV_CHECK( hipGetLastError() );
  hipLaunchKernelGGL( k_svc_compact, dim3( 1 ), dim3( 256 ), 0, s->st_flush, s->FB[0].d_desc, 0u, 0ul,
                      (u8 const *)s->d_stage, s->seg->slot_cap );
  SV_CHECK( hipGetLastError() );
  SV_CHECK( hipDeviceSynchronize() );
  s->running = 1;
  /* the ingest thread: started here, before the GPU tile's sandbox, and
     only when the process may run on two CPUs or more (a thread sharing the
     service thread's one CPU would take turns with it, the opposite of the
     point); it inherits the process's CPU set.  Without it the ingest side
     runs inside fd_verify_svc_poll (FD_VERIFY_SVC_INGEST_THREAD=0 asks for
     that on any CPU set) */
  {
    char const * e = getenv( "FD_VERIFY_SVC_INGEST_THREAD" );
    cpu_set_t cs;
    CPU_ZERO( &cs );
    int const cpus = sched_getaffinity( 0, sizeof(cs), &cs ) ? 1 : CPU_COUNT( &cs );
    if( !( e && !strcmp( e, "0" ) ) && cpus >= 2 ) {
      if( pthread_create( &s->ith, 0, svc_ingest_main, s ) ) {
        fprintf( stderr, "fd_verify_svc: the ingest thread could not start\n" );
        return -1;
      }
      s->ithread = 1;
      while( !__atomic_load_n( &s->iready, __ATOMIC_ACQUIRE ) ) __builtin_ia32_pause();
    }
  }
  fd_verify_svc_st( &s->seg->svc_state, FD_VERIFY_SVC_SVC_RUNNING );
  return 0;
}

/* validate a posted request and write its launch descriptor */
static void
svc_desc_of( fd_verify_svc_t * s, ulong t, ulong slot, ulong base, svc_desc & d ) {
  fd_verify_svc_seg_t * g = s->seg;
  fd_verify_svc_req_t const * r = fd_verify_svc_req( g, t, slot );
  memset( &d, 0, sizeof(d) );
  d.base = base; d.n = r->n; d.kind = r->kind; d.seed = r->seed; d.stage0 = svc_stage0( s, t, slot );
  d.ibase = (t * g->req_depth + slot) * g->slot_cap;
  d.state = (u64)svc_dev( s, &r->state, sizeof(ulong) );
  if( s->tile[t].client != ( r->kind == FD_VERIFY_SVC_REQ_SIGS ) ) {
    /* a client posts signature records only, a verify tile never does */
    fprintf( stderr, "fd_verify_svc: tile %lu slot %lu: request kind %lu from a %s\n", t, slot, r->kind,
             s->tile[t].client ? "client" : "verify tile" );
    abort();
  }
  if( r->kind == FD_VERIFY_SVC_REQ_RANGE ) {
    if( r->link >= FD_VERIFY_SVC_LINK_MAX || !s->link[r->link].set || !r->rr_cnt || r->rr_idx >= r->rr_cnt ||
        r->seq_cnt > s->link[r->link].depth ||
        r->n != fd_verify_svc_range_cnt( r->seq0, r->seq_cnt, r->rr_cnt, r->rr_idx ) || r->n > g->slot_cap ) {
      fprintf( stderr, "fd_verify_svc: tile %lu slot %lu: bad range request (link %lu seq0 %lu cnt %lu rr %lu/%lu n %lu)\n",
               t, slot, r->link, r->seq0, r->seq_cnt, r->rr_idx, r->rr_cnt, r->n );
      abort();
    }
    d.src = (u64)s->link[r->link].d_mcache; d.aux0 = (u64)s->link[r->link].d_base;
    d.first = fd_verify_svc_range_first( r->seq0, r->rr_cnt, r->rr_idx ); d.stride = r->rr_cnt;
    d.line_mask = s->link[r->link].depth - 1ul; d.chunk0 = s->link[r->link].chunk0; d.wmark = s->link[r->link].wmark;
  } else if( r->kind == FD_VERIFY_SVC_REQ_FRAGS || r->kind == FD_VERIFY_SVC_REQ_SIGS ) {
    if( r->n > g->frag_cap ) {
      fprintf( stderr, "fd_verify_svc: tile %lu slot %lu: %lu frags over the frag area's %lu\n", t, slot, r->n, g->frag_cap );
      abort();
    }
    d.src  = (u64)svc_dev( s, fd_verify_svc_frag( g, t, slot ), r->n * FD_VERIFY_SVC_FRAG_STRIDE );
    d.aux0 = (u64)svc_dev( s, fd_verify_svc_frag_sz( g, t, slot ), 2ul * r->n );
    d.aux1 = (u64)svc_dev( s, fd_verify_svc_frag_kind( g, t, slot ), r->n );
  } else {
    fprintf( stderr, "fd_verify_svc: tile %lu slot %lu: request kind %lu\n", t, slot, r->kind );
    abort();
  }
}

/* a verify launch over ingested requests (their descriptors were made at ingest) */
static void
svc_launch_start( fd_verify_svc_t * s, svc_launch & L ) {
  fd_verify_svc_seg_t * g = s->seg;
  ulong n = 0;
  L.nreq = 0;
  while( s->pend_head != s->pend_tail && L.nreq < SVC_REQ_MAX ) {
    svc_pend const & p = s->pend[s->pend_head % s->pend_cap];
    if( n + p.n > s->batch_max ) break;
    L.h_desc[L.nreq] = s->sdesc[p.t * g->req_depth + p.slot];
    L.h_desc[L.nreq].base = n;
    L.h_desc[L.nreq].res  = (u64)svc_dev( s, fd_verify_svc_res( g, p.t, p.slot ), sizeof(fd_verify_svc_res_t) * p.n );
    L.req[L.nreq].t = p.t; L.req[L.nreq].slot = p.slot;
    L.nreq++; n += p.n;
    s->pend_frags -= p.n; s->pend_head++;
  }
  L.n = n; L.busy = 1; L.sig = 0;
  svc_device( s->dev );
  SV_CHECK( hipEventRecord( L.ev0, L.st ) );
  hipLaunchKernelGGL( k_svc_assemble, dim3( (unsigned)((n + 255ul) / 256ul) ), dim3( 256 ), 0, L.st, L.d_desc, (u32)L.nreq,
                      n, s->d_ing_sz, s->d_ing_kind, s->d_ing_tso, L.d_in_chunk, L.d_in_sz, L.d_in_kind, L.d_tso, L.d_seed,
                      L.d_stage_chunk );
  SV_CHECK( hipGetLastError() );
  fd_txn_hip_batch_core( L.ctx, L.st, n, s->d_ing, L.d_in_chunk, L.d_in_sz, L.d_in_kind, s->d_stage, L.d_stage_chunk,
                         L.d_seed, L.d_tsz, L.d_tag, L.d_bid, L.d_first, L.d_cnt, L.d_misc, L.d_rsig, L.d_rpub,
                         L.d_rmoff, L.d_rmsz, L.rcap, L.d_rcode, L.d_tcode, L.d_fdesc );
  hipLaunchKernelGGL( k_svc_results, dim3( (unsigned)((n + 255ul) / 256ul) ), dim3( 256 ), 0, L.st, L.d_desc, (u32)L.nreq, n,
                      L.d_tsz, L.d_tag, L.d_bid, L.d_cnt, L.d_tcode, L.d_fdesc, L.d_tso );
  SV_CHECK( hipGetLastError() );
  SV_CHECK( hipEventRecord( L.ev1, L.st ) );
  s->stat[0]++; s->stat[1] += n; s->stat[2] += L.nreq;
  if( n > s->stat[15] ) s->stat[15] = n;
}

/* a signature launch over ingested client requests: records -> the
   verify's inputs (k_svc_sigrec), fd_ed25519_verify per record on the
   launch's context, codes -> the slots' result arrays (k_svc_sigres) */
static void
svc_sig_launch_start( fd_verify_svc_t * s, svc_launch & L ) {
  fd_verify_svc_seg_t * g = s->seg;
  ulong n = 0;
  L.nreq = 0;
  while( s->spend_head != s->spend_tail && L.nreq < SVC_REQ_MAX ) {
    svc_pend const & p = s->spend[s->spend_head % s->pend_cap];
    if( n + p.n > s->batch_max ) break;
    L.h_desc[L.nreq] = s->sdesc[p.t * g->req_depth + p.slot];
    L.h_desc[L.nreq].base = n;
    L.h_desc[L.nreq].res  = (u64)svc_dev( s, fd_verify_svc_res( g, p.t, p.slot ), sizeof(fd_verify_svc_res_t) * p.n );
    L.req[L.nreq].t = p.t; L.req[L.nreq].slot = p.slot;
    L.nreq++; n += p.n;
    s->spend_head++;
  }
  L.n = n; L.busy = 1; L.sig = 1;
  svc_device( s->dev );
  SV_CHECK( hipEventRecord( L.ev0, L.st ) );
  ulong wgs = (n + 3ul) / 4ul;
  if( wgs > 2048ul ) wgs = 2048ul;
  hipLaunchKernelGGL( k_svc_sigrec, dim3( (unsigned)wgs ), dim3( 256 ), 0, L.st, L.d_desc, (u32)L.nreq, n,
                      (u8 const *)s->d_ing, (u16 const *)s->d_ing_sz, s->d_stage, L.d_rsig, L.d_rpub, L.d_rmoff, L.d_rmsz );
  SV_CHECK( hipGetLastError() );
  if( fd_ed25519_hip_verify_dev( L.ctx, n, L.d_rsig, L.d_rpub, s->d_stage, L.d_rmoff, L.d_rmsz, L.d_rcode, 0, L.st ) ) {
    fprintf( stderr, "fd_verify_svc: signature launch of %lu records failed\n", n );
    abort();
  }
  hipLaunchKernelGGL( k_svc_sigres, dim3( (unsigned)((n + 255ul) / 256ul) ), dim3( 256 ), 0, L.st, L.d_desc, (u32)L.nreq, n,
                      (u16 const *)s->d_ing_sz, (signed char const *)L.d_rcode );
  SV_CHECK( hipGetLastError() );
  SV_CHECK( hipEventRecord( L.ev1, L.st ) );
  s->stat[0]++; s->stat[1] += n; s->stat[2] += L.nreq;
}

/* the gather of the newly posted requests in I (their frags into the slots'
   HBM ingest frags), on the ingest stream */
static void
svc_ingest_start( fd_verify_svc_t * s, svc_ingest & I ) {
  svc_device( s->dev );
  SV_CHECK( hipEventRecord( I.ev0, s->st_ing ) );
  ulong wgs = (I.n + 3ul) / 4ul;                            /* 4 frags per workgroup per trip */
  if( s->gather_wgs && wgs > s->gather_wgs ) wgs = s->gather_wgs;
  hipLaunchKernelGGL( k_svc_gather, dim3( (unsigned)wgs ), dim3( 256 ), 0, s->st_ing, I.d_desc,
                      (u32)I.nreq, I.n, s->d_ing, s->d_ing_sz, s->d_ing_kind, s->d_ing_tso, s->d_stage,
                      s->d_ing_ctr + (s->ing_take % SVC_ING_MAX) );
  SV_CHECK( hipGetLastError() );
  SV_CHECK( hipEventRecord( I.ev1, s->st_ing ) );
  I.busy = 1;
  s->stat[12]++;
}

/* the newly posted flushes of every tile (each tile's in order) into one
   k_svc_compact launch; 1 if it started one.  The kernel checks every
   entry's chunks against the out dcache (the host does not walk the
   entries: the service thread drives every tile) */
static int
svc_flush_batch_start( fd_verify_svc_t * s, svc_fbatch & F ) {
  fd_verify_svc_seg_t * g = s->seg;
  F.nf = 0; F.n = 0;
  for( ulong t = 0; t < g->tile_cnt && F.nf < SVC_FB_FLUSH_MAX; t++ ) {
    svc_tile & T = s->tile[t];
    if( T.client ) continue;
    fd_verify_svc_tile_t * b = fd_verify_svc_tile( g, t );
    ulong const post = fd_verify_svc_ld( &b->flush_post );
    while( T.flush_take < post && F.nf < SVC_FB_FLUSH_MAX ) {
      fd_verify_svc_flush_t const * f = &b->flush[T.flush_take % FD_VERIFY_SVC_FLUSH_DEPTH];
      if( f->slot >= g->req_depth || f->lo > f->hi || f->hi > g->slot_cap ) {
        fprintf( stderr, "fd_verify_svc: tile %lu: bad flush (slot %lu [%lu,%lu))\n", t, f->slot, f->lo, f->hi );
        abort();
      }
      ulong const m = f->hi - f->lo;
      svc_fdesc & d = F.h_desc[F.nf];
      d.base = F.n;
      d.out = m ? (u64)svc_dev( s, fd_verify_svc_out( g, t, f->slot ) + f->lo, m * sizeof(fd_verify_svc_out_t) ) : 0ul;
      d.stage0 = svc_stage0( s, t, f->slot ); d.dcache = (u64)T.d_out;
      d.delta = (long)(T.chunk_base - T.h_out);            /* dcache offset of chunk c: 64 c + delta */
      d.out_sz = T.out_sz; d.err = (u64)T.d_err; d.rsv = 0;
      F.t[F.nf] = (u8)t;
      F.nf++; F.n += m;
      T.flush_take++;
      s->stat[3]++; s->stat[4] += m;
    }
  }
  if( !F.nf ) return 0;
  svc_device( s->dev );
  if( F.n ) {
    ulong wgs = (F.n + 3ul) / 4ul;
    if( s->flush_wgs && wgs > s->flush_wgs ) wgs = s->flush_wgs;
    hipLaunchKernelGGL( k_svc_compact, dim3( (unsigned)wgs ), dim3( 256 ), 0, s->st_flush, F.d_desc, F.nf, F.n,
                        (u8 const *)s->d_stage, g->slot_cap );
    SV_CHECK( hipGetLastError() );
    s->stat[6]++;
  }
  SV_CHECK( hipEventRecord( F.ev, s->st_flush ) );
  F.busy = 1;
  return 1;
}

/* the ingest side of a poll: 1b. finished gathers, in order (their
   requests' frags are in HBM, the tiles may reuse the link space) into the
   handoff ring; 2. newly posted requests, in each tile's ring order, into
   one gather batch (a request waits while every batch is busy).  Runs on
   the ingest thread, or inside fd_verify_svc_poll without one; it alone
   touches the ING ring, the tiles' take counters, sdesc and stat[12..14] */
static int
svc_ingest_step( fd_verify_svc_t * s ) {
  fd_verify_svc_seg_t * g = s->seg;
  int did = 0;
  long const now0 = svc_now_ns();
  ulong tail = s->ih_tail;
  while( s->ing_fin < s->ing_take ) {
    svc_ingest & I = s->ING[s->ing_fin % SVC_ING_MAX];
    hipError_t e = hipEventQuery( I.ev1 );
    if( e == hipErrorNotReady ) break;
    SV_CHECK( e );
    float ms = 0.f;
    SV_CHECK( hipEventElapsedTime( &ms, I.ev0, I.ev1 ) );
    s->stat[13] += (ulong)((double)ms * 1e6);
    /* the gather's last workgroup has stored INGESTED into each slot (the
       tiles learn it from the GPU, not from this turn); here they go to the
       launch queues */
    for( ulong r = 0; r < I.nreq; r++ ) {
      svc_pend & p = s->ih[tail % s->ih_cap];
      p.t = I.req[r].t; p.slot = I.req[r].slot; p.n = I.h_desc[r].n; p.seen = now0;
      p.sig = I.h_desc[r].kind == FD_VERIFY_SVC_REQ_SIGS;
      tail++;
    }
    I.busy = 0; s->ing_fin++; did = 1;
  }
  __atomic_store_n( &s->ih_tail, tail, __ATOMIC_RELEASE );
  long const p1 = svc_now_ns();
  /* a range request holds its link until its gather has read it */
  if( s->ing_take - s->ing_fin < SVC_ING_MAX ) {
    svc_ingest & I = s->ING[s->ing_take % SVC_ING_MAX];
    I.nreq = 0; I.n = 0;
    for( ulong t = 0; t < g->tile_cnt && I.nreq < SVC_REQ_MAX; t++ ) {
      svc_tile & T = s->tile[t];
      while( I.nreq < SVC_REQ_MAX ) {
        ulong slot = T.take & (g->req_depth - 1ul);
        fd_verify_svc_req_t * q = fd_verify_svc_req( g, t, slot );
        if( fd_verify_svc_ld( &q->state ) != FD_VERIFY_SVC_POSTED ) break;
        if( q->id + g->req_depth == T.take ) break;          /* the slot's previous request, still on the GPU */
        if( q->id != T.take ) {
          fprintf( stderr, "fd_verify_svc: tile %lu posted request %lu in slot %lu, expected %lu\n", t, q->id, slot, T.take );
          abort();
        }
        T.take++; did = 1;
        if( !q->n ) {                                        /* nothing to verify: results at once */
          q->batch_frags = 0; fd_verify_svc_st( &q->state, FD_VERIFY_SVC_RESULTS );
          continue;
        }
        svc_desc & d = s->sdesc[t * g->req_depth + slot];
        svc_desc_of( s, t, slot, I.n, d );
        I.h_desc[I.nreq] = d;
        I.req[I.nreq].t = t; I.req[I.nreq].slot = slot;
        I.nreq++; I.n += q->n;
      }
    }
    if( I.nreq ) { svc_ingest_start( s, I ); s->ing_take++; }
  }
  s->stat[14] += (ulong)(svc_now_ns() - p1);
  return did;
}

static void *
svc_ingest_main( void * arg ) {
  fd_verify_svc_t * s = (fd_verify_svc_t *)arg;
  /* the thread's first HIP calls (the runtime's per-thread setup), an empty
     gather, an event and its query, and its first malloc (its arena) happen
     here, before fd_verify_svc_run returns and the GPU tile enters its
     sandbox: made after it, the setup's calls met the seccomp filter (one
     bench run of r06l ended in SIGSYS) */
  svc_device( s->dev );
  free( malloc( 4096 ) );
  hipLaunchKernelGGL( k_svc_gather, dim3( 1 ), dim3( 256 ), 0, s->st_ing, s->ING[0].d_desc, 0u, 0ul, s->d_ing, s->d_ing_sz,
                      s->d_ing_kind, s->d_ing_tso, s->d_stage, (u32 *)0 );
  SV_CHECK( hipGetLastError() );
  SV_CHECK( hipEventRecord( s->ING[0].ev0, s->st_ing ) );
  SV_CHECK( hipEventRecord( s->ING[0].ev1, s->st_ing ) );
  SV_CHECK( hipStreamSynchronize( s->st_ing ) );
  SV_CHECK( hipEventQuery( s->ING[0].ev1 ) );
  float ms = 0.f;
  SV_CHECK( hipEventElapsedTime( &ms, s->ING[0].ev0, s->ING[0].ev1 ) );
  __atomic_store_n( &s->iready, 1, __ATOMIC_RELEASE );
  while( !__atomic_load_n( &s->istop, __ATOMIC_ACQUIRE ) )
    if( !svc_ingest_step( s ) ) __builtin_ia32_pause();
  __atomic_store_n( &s->iexited, 1, __ATOMIC_RELEASE );
  return 0;
}

extern "C" int
fd_verify_svc_poll( fd_verify_svc_t * s ) {
  fd_verify_svc_seg_t * g = s->seg;
  int did = 0;
  long const p0 = svc_now_ns();
  svc_device( s->dev );
  g->svc_heartbeat++;
  s->stat[11]++;
  if( !(s->stat[11] & 63ul) ) {
    ulong c[4] = { 0ul, 0ul, 0ul, 0ul };
    for( ulong t = 0; t < g->tile_cnt; t++ )
      for( ulong k = 0; k < g->req_depth; k++ ) {
        ulong st = fd_verify_svc_ld( &fd_verify_svc_req( g, t, k )->state );
        c[st == FD_VERIFY_SVC_POSTED ? 0 : st == FD_VERIFY_SVC_INGESTED ? 1 : st == FD_VERIFY_SVC_RESULTS ? 2 : 3]++;
      }
    ulong launched = 0;
    for( ulong k = 0; k < s->inflight; k++ ) if( s->L[k].busy ) launched += s->L[k].nreq;
    if( c[3] < g->tile_cnt * g->req_depth ) {                  /* only while some slot is in use */
      s->occ[0]++; s->occ[1] += c[0]; s->occ[2] += c[1] - launched; s->occ[3] += launched; s->occ[4] += c[2];
      s->occ[5] += c[3];
    }
  }
  /* 1. finished verify launches: their slots' results are in the segment */
  ulong busy = 0;
  for( ulong k = 0; k < s->inflight; k++ ) {
    svc_launch & L = s->L[k];
    if( !L.busy ) continue;
    hipError_t e = hipEventQuery( L.ev1 );
    if( e == hipErrorNotReady ) {
      /* a launch that never ends (a stream sharing a hardware queue behind
         a kernel that never ends would) ends the service loudly, not silently */
      if( p0 - s->launch_t0[k] > 20000000000L ) {
        fprintf( stderr, "fd_verify_svc: verify launch %lu (%lu frags) not done after 20 s\n", k, L.n );
        abort();
      }
      busy++; continue;
    }
    SV_CHECK( e );
    float ms = 0.f;
    SV_CHECK( hipEventElapsedTime( &ms, L.ev0, L.ev1 ) );
    s->stat[7] += (ulong)((double)ms * 1e6);
    for( ulong r = 0; r < L.nreq; r++ ) {
      fd_verify_svc_req_t * q = fd_verify_svc_req( g, L.req[r].t, L.req[r].slot );
      q->batch_frags = L.n;
      fd_verify_svc_st( &q->state, FD_VERIFY_SVC_RESULTS );
    }
    L.busy = 0; did = 1;
  }
  long const p1 = svc_now_ns();
  s->stat[10] += (ulong)(p1 - p0);
  /* 1b, 2: the ingest side, here when it has no thread of its own */
  if( !s->ithread ) did |= svc_ingest_step( s );
  /* ingested requests join the launch queues (txn frags merge; signature
     requests ride their own launches) */
  {
    ulong const tail = __atomic_load_n( &s->ih_tail, __ATOMIC_ACQUIRE );
    for( ; s->ih_head < tail; s->ih_head++ ) {
      svc_pend const & h = s->ih[s->ih_head % s->ih_cap];
      if( h.sig ) { s->spend[s->spend_tail % s->pend_cap] = h; s->spend_tail++; }
      else        { s->pend[s->pend_tail % s->pend_cap] = h; s->pend_tail++; s->pend_frags += h.n; }
      did = 1;
    }
  }
  long const p2 = svc_now_ns();
  /* 3. flushes: retire in order, start the newly posted */
  while( s->fb_fin < s->fb_take ) {
    svc_fbatch & F = s->FB[s->fb_fin % SVC_FB_MAX];
    hipError_t e = hipEventQuery( F.ev );
    if( e == hipErrorNotReady ) break;
    SV_CHECK( e );
    for( u32 i = 0; i < F.nf; i++ ) {
      ulong const t = F.t[i];
      svc_tile & T = s->tile[t];
      if( *(volatile u32 *)T.h_err ) {
        fprintf( stderr, "fd_verify_svc: tile %lu: a flush entry's chunks lie outside the out dcache\n", t );
        abort();
      }
      T.flush_fin++;
      fd_verify_svc_st( &fd_verify_svc_tile( g, t )->flush_done, T.flush_fin );
    }
    F.busy = 0; s->fb_fin++; did = 1;
  }
  for( ulong t = 0; t < g->tile_cnt; t++ )
    if( s->tile[t].client && fd_verify_svc_ld( &fd_verify_svc_tile( g, t )->flush_post ) ) {
      fprintf( stderr, "fd_verify_svc: tile %lu is a client and posted a flush\n", t );
      abort();
    }
  if( s->fb_take - s->fb_fin < SVC_FB_MAX ) {
    if( svc_flush_batch_start( s, s->FB[s->fb_take % SVC_FB_MAX] ) ) { s->fb_take++; did = 1; }
  }
  long const now = svc_now_ns();
  s->stat[9] += (ulong)(now - p2);
  /* 4. a verify launch: when the ingested frags fill its merge target, or
     the oldest has waited merge_wait_ns, or (the GPU idle) merge_idle_ns --
     large launches while the GPU is busy (a 55 K-signature launch runs ~one
     wave per SIMD and costs 3x per signature), little added
     latency while it is not */
  /* 4a. signature requests (clients: a FEC set's root, a replay batch)
     launch as soon as a launch slot is free: they are few and wait on
     their caller, so no merge target */
  while( s->spend_head != s->spend_tail && busy < s->inflight ) {
    ulong k = 0;
    while( s->L[k].busy ) k++;
    long const l0 = svc_now_ns();
    s->launch_t0[k] = l0;
    svc_sig_launch_start( s, s->L[k] );
    s->stat[8] += (ulong)(svc_now_ns() - l0);
    busy++; did = 1;
  }
  while( s->pend_head != s->pend_tail && busy < s->inflight ) {
    long waited = now - s->pend[s->pend_head % s->pend_cap].seen;
    bool ready = s->pend_frags >= s->merge_min || waited >= s->merge_wait_ns || ( !busy && waited >= s->merge_idle_ns );
    if( !ready ) break;
    ulong k = 0;
    while( s->L[k].busy ) k++;
    long const l0 = svc_now_ns();
    s->launch_t0[k] = l0;
    svc_launch_start( s, s->L[k] );
    s->stat[8] += (ulong)(svc_now_ns() - l0);
    busy++; did = 1;
  }
  return did;
}

extern "C" void
fd_verify_svc_stats( fd_verify_svc_t const * s, ulong out[16] ) {
  for( int k = 0; k < 16; k++ ) out[k] = s->stat[k];
}

/* one line of the service's state, for a stalled run's log (svc_run.c
   SVC_DEBUG_S) */
extern "C" int
fd_verify_svc_debug( fd_verify_svc_t const * s, char * buf, ulong sz ) {
  fd_verify_svc_seg_t const * g = s->seg;
  int n = snprintf( buf, sz, "polls %lu launches %lu frags %lu pend %lu/%lu", s->stat[11], s->stat[0], s->stat[1],
                    s->pend_tail - s->pend_head, s->pend_frags );
  for( ulong k = 0; k < s->inflight && n > 0 && (ulong)n < sz; k++ )
    n += snprintf( buf + n, sz - (ulong)n, " L%lu:%d/%lu", k, s->L[k].busy, s->L[k].n );
  for( ulong t = 0; t < g->tile_cnt && t < 4ul && n > 0 && (ulong)n < sz; t++ ) {
    ulong st[4] = { 0, 0, 0, 0 };
    for( ulong k = 0; k < g->req_depth; k++ ) st[__atomic_load_n( &fd_verify_svc_req( (fd_verify_svc_seg_t *)g, t, k )->state, __ATOMIC_ACQUIRE ) & 3ul]++;
    /* take: the ingest side's counter (its thread's, when it has one) */
    n += snprintf( buf + n, sz - (ulong)n, " t%lu[take %lu free %lu posted %lu results %lu ingested %lu]", t,
                   __atomic_load_n( &s->tile[t].take, __ATOMIC_RELAXED ), st[0], st[1], st[2], st[3] );
  }
  return n;
}

extern "C" void
fd_verify_svc_occupancy( fd_verify_svc_t const * s, ulong out[6] ) {
  for( int k = 0; k < 6; k++ ) out[k] = s->occ[k];
}

/* Teardown waits for each stream's work with a deadline, stage by stage,
   so that a stuck shutdown says where it is stuck (a run's
   service did not finish its shutdown in 60 s and left no trace of where;
   hipDeviceSynchronize blocks without one).  A stage still running after
   2 s is named on stderr, after 30 s the process aborts naming it. */
static void
svc_drain( hipStream_t st, char const * what, ulong idx ) {
  hipEvent_t ev;
  /* each stage is named before its first HIP call: in rounds 5 and 6, with
     CU-masked verify streams in the process (a configuration since removed),
     teardown hung with nothing said after "teardown" (profiles/r06/teardown) */
  if( getenv( "FD_VERIFY_SVC_TEARDOWN_LOG" ) ) fprintf( stderr, "fd_verify_svc: teardown: %s %lu\n", what, idx );
  SV_CHECK( hipEventCreateWithFlags( &ev, hipEventDisableTiming ) );
  if( getenv( "FD_VERIFY_SVC_TEARDOWN_LOG" ) ) fprintf( stderr, "fd_verify_svc: teardown: %s %lu: event created\n", what, idx );
  SV_CHECK( hipEventRecord( ev, st ) );
  if( getenv( "FD_VERIFY_SVC_TEARDOWN_LOG" ) ) fprintf( stderr, "fd_verify_svc: teardown: %s %lu: event recorded\n", what, idx );
  long const t0 = svc_now_ns();
  int warned = 0;
  for( ;; ) {
    hipError_t e = hipEventQuery( ev );
    if( e == hipSuccess ) break;
    if( e != hipErrorNotReady ) {
      fprintf( stderr, "fd_verify_svc: teardown: %s %lu: %s\n", what, idx, hipGetErrorString( e ) );
      abort();
    }
    long const dt = svc_now_ns() - t0;
    if( dt > 2000000000L && !warned ) {
      warned = 1;
      fprintf( stderr, "fd_verify_svc: teardown: %s %lu still running after 2 s\n", what, idx );
    }
    if( dt > 30000000000L ) {
      fprintf( stderr, "fd_verify_svc: teardown: %s %lu not done after 30 s\n", what, idx );
      abort();
    }
    struct timespec ts = { 0, 100000L };
    nanosleep( &ts, 0 );
  }
  if( warned ) fprintf( stderr, "fd_verify_svc: teardown: %s %lu done after %.1f s\n", what, idx, 1e-9 * (double)(svc_now_ns() - t0) );
  (void)hipEventDestroy( ev );
}

extern "C" void
fd_verify_svc_delete( fd_verify_svc_t * s ) {
  if( !s ) return;
  /* no HIP call before the ingest thread has stopped: a call that takes a
     runtime lock the thread holds inside a blocked HIP call would hang here
     with nothing said (profiles/r06/teardown: in a run with CU-masked verify
     streams nothing came after "teardown" for 60 s) */
  if( getenv( "FD_VERIFY_SVC_TEARDOWN_LOG" ) ) fprintf( stderr, "fd_verify_svc: teardown: begin (ingest thread %d)\n", s->ithread );
  if( s->ithread ) {                          /* no new gathers from here on (the stream drains below) */
    __atomic_store_n( &s->istop, 1, __ATOMIC_RELEASE );
    /* a thread held inside a HIP call would hold pthread_join silently: the
       wait is staged as the streams' are (named after 2 s, abort after 30 s) */
    long const t0 = svc_now_ns();
    int warned = 0;
    while( !__atomic_load_n( &s->iexited, __ATOMIC_ACQUIRE ) ) {
      long const dt = svc_now_ns() - t0;
      if( dt > 2000000000L && !warned ) {
        warned = 1;
        fprintf( stderr, "fd_verify_svc: teardown: the ingest thread still in a HIP call after 2 s (gathers %lu started, "
                 "%lu retired)\n", s->ing_take, s->ing_fin );
      }
      if( dt > 30000000000L ) { fprintf( stderr, "fd_verify_svc: teardown: the ingest thread not done after 30 s\n" ); abort(); }
      struct timespec ts = { 0, 100000L };
      nanosleep( &ts, 0 );
    }
    (void)pthread_join( s->ith, 0 );
    s->ithread = 0;
  }
  svc_device( s->dev );                       /* the service thread's device (set by its polls already) */
  for( ulong k = 0; k < s->inflight; k++ ) if( s->L[k].ctx ) svc_drain( s->L[k].st, "verify launch stream", k );
  svc_drain( s->st_flush, "flush stream", 0ul );
  svc_drain( s->st_ing, "ingest stream", 0ul );
  /* the null stream (the runtime's memsets) the same way, never
     hipDeviceSynchronize, which blocks with no deadline: in the r05m and
     r06o shutdown hangs (a CU-masked stream in the process, a configuration
     since removed) it never returned although every stream above had
     drained (profiles/r06/teardown) */
  svc_drain( 0, "null stream", 0ul );
  for( ulong k = 0; k < SVC_LAUNCH_MAX; k++ ) launch_free( s->L[k] );
  for( ulong t = 0; t < FD_VERIFY_SVC_TILE_MAX; t++ )
    if( s->tile[t].h_err ) (void)hipHostFree( s->tile[t].h_err );
  (void)hipFree( s->d_stage );
  (void)hipFree( s->d_ing ); (void)hipFree( s->d_ing_sz ); (void)hipFree( s->d_ing_kind ); (void)hipFree( s->d_ing_tso );
  (void)hipFree( s->d_ing_ctr );
  for( ulong k = 0; k < SVC_ING_MAX; k++ ) {
    svc_ingest & I = s->ING[k];
    if( !I.h_desc ) continue;
    (void)hipHostFree( I.h_desc ); (void)hipEventDestroy( I.ev0 ); (void)hipEventDestroy( I.ev1 );
  }
  (void)hipStreamDestroy( s->st_ing );
  for( ulong k = 0; k < SVC_FB_MAX; k++ ) {
    if( !s->FB[k].h_desc ) continue;
    (void)hipHostFree( s->FB[k].h_desc ); (void)hipEventDestroy( s->FB[k].ev );
  }
  (void)hipStreamDestroy( s->st_flush );
  free( s->sdesc );
  for( ulong k = 0; k < s->nreg; k++ ) (void)hipHostUnregister( s->reg[k].h );
  fd_verify_svc_st( &s->seg->svc_state, FD_VERIFY_SVC_SVC_STOPPED );
  free( s->pend ); free( s->spend ); free( s->ih );
  free( s );
}
