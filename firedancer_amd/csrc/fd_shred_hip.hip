/* Shred Merkle roots and FEC-set verification from raw shreds on gfx950:
   include/fd_replay_hip.h, shred section.

   The reference's FEC resolver hashes the Merkle-protected part of every
   shred to its set's root (fd_shred_merkle_root, src/ballet/shred/
   fd_shred.c:108-131: one SHA-256 over about 1.1 KB, then one 66-byte merge
   per proof level, src/ballet/bmtree/fd_bmtree.c:52-142) and then checks one
   signature per set (src/disco/shred/fd_fec_resolver.c:476).  Here both
   halves run on the device, in one stream-ordered sequence:

     k_shred_roots    one shred per lane: header checks, the leaf hash through
                      the LDS-staged SHA-256 (fd_sha256_dev.h), the proof walk
                      in registers
     k_shred_pick     one representative per distinct (signature, root,
                      leader key) triple, through an open-addressing table
     fd_ed25519_hip_verify_dev_count over the representatives (count on the
                      device)
     k_shred_scatter  every shred gets its representative's code

   No kernel waits for another workgroup. */

#include "../../include/fd_replay_hip.h"
#include "fd_sha256_dev.h"

#include <hip/hip_runtime.h>
#include <random>
#include <stdio.h>
#include <stdlib.h>

#define SH_CHECK( x ) do {                                                            \
    hipError_t e_ = (x);                                                               \
    if( e_ != hipSuccess ) {                                                           \
      fprintf( stderr, "fd_shred_hip: %s failed at %s:%d: %s\n", #x, __FILE__,       \
               __LINE__, hipGetErrorString( e_ ) );                                    \
      abort();                                                                         \
    }                                                                                  \
  } while( 0 )

/* "\x00SOLANA_MERKLE_SHREDS_LEAF" and "\x01SOLANA_MERKLE_SHREDS_NODE" (fd_bmtree.c:52-93) as little-endian words */
static constexpr u32 pre_word( char const * s, int k ) {
  u32 w = 0u;
  for( int j=0; j<4; j++ ) if( 4*k + j < 26 ) w |= (u32)(u8)s[4*k+j] << (8*j);
  return w;
}
#define PRE_WORDS( s ) { pre_word( s, 0 ), pre_word( s, 1 ), pre_word( s, 2 ), pre_word( s, 3 ), pre_word( s, 4 ), \
                         pre_word( s, 5 ), pre_word( s, 6 ) }
static __device__ const u32 PRE_LEAF[7] = PRE_WORDS( "\x00SOLANA_MERKLE_SHREDS_LEAF" );
static __device__ const u32 PRE_NODE[7] = PRE_WORDS( "\x01SOLANA_MERKLE_SHREDS_NODE" );

#define SHA256_WAVE_WORDS (64u*SHA256_WIN_WORDS)

/* ---- plain SHA-256 of n messages ----------------------------------------- */

__global__ __launch_bounds__(256)
void k_sha256_batch( ulong n, uchar const * __restrict__ pool, uint const * __restrict__ off,
                     uint const * __restrict__ sz, uchar * __restrict__ hash ) {
  __shared__ __attribute__((aligned(16))) u32 lds_msg_all[4*SHA256_WAVE_WORDS];
  __shared__ u64 lds_meta_all[4*64];
  ulong wave0 = (ulong)blockIdx.x * 256ul + (threadIdx.x & ~63u);
  if( wave0 >= n ) return;                          /* wave-uniform: the hash below needs all 64 lanes */
  u32 lane = threadIdx.x & 63u;
  ulong i = wave0 + lane;
  bool live = i < n;
  u32 st[8];
  sha256_coop<0u>( st, nullptr, pool + (live ? off[i] : 0u), live ? sz[i] : 0u, live,
                   lds_msg_all + SHA256_WAVE_WORDS*(threadIdx.x >> 6), lds_meta_all + 64*(threadIdx.x >> 6), lane );
  if( !live ) return;
  uint4 * o = (uint4 *)(hash + 32ul*i);
  o[0] = make_uint4( bswap32( st[0] ), bswap32( st[1] ), bswap32( st[2] ), bswap32( st[3] ) );
  o[1] = make_uint4( bswap32( st[4] ), bswap32( st[5] ), bswap32( st[6] ), bswap32( st[7] ) );
}

/* ---- roots ------------------------------------------------------------------ */

DEV u32 ld_u16( u8 const * p ) { return (u32)p[0] | ((u32)p[1] << 8); }
DEV u32 ld_u32( u8 const * p ) { return ld_u16( p ) | (ld_u16( p + 2 ) << 16); }

/* 4 bytes at any address as a little-endian word, from the two aligned words that hold them (reads up to the
   4-byte boundary after p+3) */
DEV u32 ld_u32_unal( u8 const * p ) {
  uintptr_t a = (uintptr_t)p;
  u32 const * q = (u32 const *)(a & ~(uintptr_t)3);
  u32 sh = (u32)(a & 3u) * 8u;
  u32 w0 = q[0];
  u32 w1 = sh ? q[1] : 0u;
  return __builtin_amdgcn_alignbit( w1, w0, sh );
}

/* struct fd_shred (src/ballet/shred/fd_shred.h:185-257), little-endian, packed */
#define SHRED_OFF_VARIANT     0x40u
#define SHRED_OFF_IDX         0x49u
#define SHRED_OFF_FEC_SET_IDX 0x4fu
#define SHRED_OFF_DATA_CNT    0x53u
#define SHRED_OFF_CODE_CNT    0x55u
#define SHRED_OFF_CODE_IDX    0x57u
#define SHRED_MIN_SZ          1203u   /* FD_SHRED_MIN_SZ: every data shred */
#define SHRED_MAX_SZ          1228u   /* FD_SHRED_MAX_SZ: every code shred */
#define SHRED_IN_TYPE_MAX     67u     /* FD_REEDSOL_DATA_SHREDS_MAX = FD_REEDSOL_PARITY_SHREDS_MAX */
#define SHRED_DEPTH_MAX       9u      /* FD_SHRED_MERKLE_LAYER_CNT - 1 */

__global__ __launch_bounds__(256)
void k_shred_roots( ulong n, uchar const * __restrict__ pool, uint const * __restrict__ off,
                    uint const * __restrict__ sz, uchar * __restrict__ roots, uchar * __restrict__ flags ) {
  __shared__ __attribute__((aligned(16))) u32 lds_msg_all[4*SHA256_WAVE_WORDS];
  __shared__ u64 lds_meta_all[4*64];
  ulong wave0 = (ulong)blockIdx.x * 256ul + (threadIdx.x & ~63u);
  if( wave0 >= n ) return;                          /* wave-uniform */
  u32 lane = threadIdx.x & 63u;
  ulong i = wave0 + lane;
  bool live = i < n;
  u8 const * p = pool + (live ? off[i] : 0u);
  u32 s = live ? sz[i] : 0u;

  bool ok = false;
  u32 d = 0u, P = 0u, sidx = 0u;
  if( s >= SHRED_MIN_SZ ) {                          /* every header field lies below 0x59 */
    u32 variant = p[SHRED_OFF_VARIANT];
    u32 type = variant & 0xf0u;
    d = variant & 0x0fu;
    bool data = (type & 0xC0u) == 0x80u;
    bool merkle = type == 0x80u || type == 0x90u || type == 0xB0u || type == 0x40u || type == 0x60u || type == 0x70u;
    u32 r = (type == 0xB0u || type == 0x70u) ? 1u : 0u;
    u32 in_idx;
    ok = merkle && d <= SHRED_DEPTH_MAX && s >= (data ? SHRED_MIN_SZ : SHRED_MAX_SZ);
    if( data ) {
      in_idx = ld_u32( p + SHRED_OFF_IDX ) - ld_u32( p + SHRED_OFF_FEC_SET_IDX );
      sidx = in_idx;
    } else {
      u32 data_cnt = ld_u16( p + SHRED_OFF_DATA_CNT ), code_cnt = ld_u16( p + SHRED_OFF_CODE_CNT );
      in_idx = ld_u16( p + SHRED_OFF_CODE_IDX );
      sidx = in_idx + data_cnt;
      ok = ok && data_cnt >= 1u && data_cnt <= SHRED_IN_TYPE_MAX && code_cnt >= 1u && code_cnt <= SHRED_IN_TYPE_MAX;
    }
    ok = ok && in_idx < SHRED_IN_TYPE_MAX && sidx < (1u << d);
    if( !ok ) d = 0u;
    P = (data ? 1139u : 1164u) - 20u*d - 64u*r;      /* the leaf covers shred[ 64, 64+P ) */
  }

  u32 st[8];
  sha256_coop<26u>( st, PRE_LEAF, p + 64, P, ok, lds_msg_all + SHA256_WAVE_WORDS*(threadIdx.x >> 6),
                    lds_meta_all + 64*(threadIdx.x >> 6), lane );
  if( !live ) return;
  if( ok ) {
    u8 const * proof = p + 64u + P;                  /* d siblings of 20 bytes, leaf level first */
    #pragma unroll 1
    for( u32 k=0; k<d; k++ ) {
      u32 node[5], sib[5], L[5], R[5];
      #pragma unroll
      for( int j=0; j<5; j++ ) { node[j] = bswap32( st[j] ); sib[j] = ld_u32_unal( proof + 20u*k + 4u*(u32)j ); }
      bool right = (sidx >> k) & 1u;                 /* this node is its parent's right child */
      #pragma unroll
      for( int j=0; j<5; j++ ) { L[j] = right ? sib[j] : node[j]; R[j] = right ? node[j] : sib[j]; }
      sha256_merge20( st, PRE_NODE, L, R );
    }
  }
  uint4 * o = (uint4 *)(roots + 32ul*i);
  o[0] = ok ? make_uint4( bswap32( st[0] ), bswap32( st[1] ), bswap32( st[2] ), bswap32( st[3] ) ) : make_uint4( 0u, 0u, 0u, 0u );
  o[1] = ok ? make_uint4( bswap32( st[4] ), bswap32( st[5] ), bswap32( st[6] ), bswap32( st[7] ) ) : make_uint4( 0u, 0u, 0u, 0u );
  flags[i] = ok ? (uchar)1 : (uchar)0;
}

/* ---- one representative per distinct (signature, root, leader key) --------- */

#define PICK_EMPTY 0xffffffffu

DEV bool triple_eq( u8 const * sig_a, u8 const * sig_b, uint4 const * root_a, uint4 const * root_b,
                    uint4 const * pub_a, uint4 const * pub_b ) {
  u32 diff = 0u;
  #pragma unroll
  for( int q=0; q<2; q++ ) {
    uint4 x = root_a[q], y = root_b[q];
    diff |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
    x = pub_a[q]; y = pub_b[q];
    diff |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
  }
  if( diff ) return false;
  #pragma unroll 4
  for( u32 k=0; k<16u; k++ ) diff |= ld_u32_unal( sig_a + 4u*k ) ^ ld_u32_unal( sig_b + 4u*k );
  return !diff;
}

/* stat[0]: representatives so far (the verify's record count); stat[1]: shreds with a root.
   rep[i]: the shred whose table entry stands for shred i's triple; slot[k]: that shred's record. */
__global__ __launch_bounds__(256)
void k_shred_pick( ulong n, uchar const * __restrict__ pool, uint const * __restrict__ off,
                   uchar const * __restrict__ pubs, uchar const * __restrict__ roots, uchar const * __restrict__ flags,
                   u32 * __restrict__ tab, u32 tmask, u32 salt, u32 * __restrict__ stat, u32 * __restrict__ rep,
                   u32 * __restrict__ slot, uchar * __restrict__ rroot, uchar * __restrict__ rsig,
                   uchar * __restrict__ rpub, u32 * __restrict__ rmoff, u32 * __restrict__ rmsz ) {
  ulong i = (ulong)blockIdx.x * 256ul + threadIdx.x;
  bool f = i < n && flags[i];
  unsigned long long m = __ballot( f );
  if( (threadIdx.x & 63u) == 0u && m ) atomicAdd( stat + 1, (u32)__popcll( m ) );
  if( !f ) return;
  u8 const * sig = pool + off[i];
  uint4 const * root = (uint4 const *)(roots + 32ul*i), * pub = (uint4 const *)(pubs + 32ul*i);
  /* every byte of the triple goes into the slot hash, keyed by the handle's salt: a sender chooses signatures and
     payloads freely, and could otherwise aim all shreds of a burst at one probe chain */
  uint4 r0 = root[0], r1 = root[1], p0 = pub[0], p1 = pub[1];
  u32 w[16] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w };
  u32 h = salt;
  #pragma unroll
  for( int k=0; k<16; k++ ) { h = (h ^ w[k]) * 0x9e3779b1u; h ^= h >> 15; }
  #pragma unroll 4
  for( u32 k=0; k<16u; k++ ) { h = (h ^ ld_u32_unal( sig + 4u*k )) * 0x85ebca6bu; h ^= h >> 13; }
  h *= 0xc2b2ae35u; h ^= h >> 16;
  for( u32 probe=0u; probe<=tmask; probe++ ) {
    u32 t = (h + probe) & tmask;
    u32 prev = atomicCAS( tab + t, PICK_EMPTY, (u32)i );
    if( prev == PICK_EMPTY ) {                       /* this shred stands for its triple */
      u32 j = atomicAdd( stat, 1u );
      rep[i] = (u32)i; slot[i] = j;
      uint4 * qr = (uint4 *)(rroot + 32ul*j), * qp = (uint4 *)(rpub + 32ul*j);
      qr[0] = r0; qr[1] = r1; qp[0] = p0; qp[1] = p1;
      u32 * qs = (u32 *)(rsig + 64ul*j);
      #pragma unroll 4
      for( u32 k=0; k<16u; k++ ) qs[k] = ld_u32_unal( sig + 4u*k );
      rmoff[j] = 32u*j; rmsz[j] = 32u;
      return;
    }
    if( triple_eq( sig, pool + off[prev], root, (uint4 const *)(roots + 32ul*prev), pub,
                   (uint4 const *)(pubs + 32ul*prev) ) ) {
      rep[i] = prev;
      return;
    }
  }
  /* not reached: the table has at least twice as many entries as shreds */
}

__global__ __launch_bounds__(256)
void k_shred_scatter( ulong n, uchar const * __restrict__ flags, u32 const * __restrict__ rep,
                      u32 const * __restrict__ slot, signed char const * __restrict__ rcode,
                      signed char * __restrict__ codes ) {
  ulong i = (ulong)blockIdx.x * 256ul + threadIdx.x;
  if( i >= n ) return;
  codes[i] = flags[i] ? rcode[ slot[ rep[i] ] ] : (signed char)FD_SHRED_HIP_NO_ROOT;
}

/* ---- host ------------------------------------------------------------------- */

struct fd_shred_hip {
  fd_ed25519_hip_ctx_t * ctx;
  ulong   n_max, tsize;
  u32     salt;                                    /* keys k_shred_pick's slot hash */
  u32 *   d_tab; u32 * d_stat; u32 * d_rep; u32 * d_slot;
  uchar * d_rroot; uchar * d_rsig; uchar * d_rpub; u32 * d_rmoff; u32 * d_rmsz; signed char * d_rcode;
  hipEvent_t ev_last; int ev_used;
};

static void
launch_roots( hipStream_t st, ulong n, uchar const * d_pool, uint const * d_off, uint const * d_sz, uchar * d_roots,
              uchar * d_flags ) {
  hipLaunchKernelGGL( k_shred_roots, dim3( (unsigned)((n + 255ul)/256ul) ), dim3( 256 ), 0, st, n, d_pool, d_off, d_sz,
                      d_roots, d_flags );
  SH_CHECK( hipGetLastError() );
}

extern "C" {

int
fd_sha256_hip_batch_dev( fd_ed25519_hip_ctx_t * ctx, ulong n, uchar const * d_pool, uint const * d_off,
                         uint const * d_sz, uchar * d_hash, void * stream ) {
  if( !n ) return 0;
  if( n > (ulong)UINT32_MAX ) return -1;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)fd_ed25519_hip_ctx_stream( ctx );
  SH_CHECK( hipSetDevice( fd_ed25519_hip_ctx_device( ctx ) ) );
  hipLaunchKernelGGL( k_sha256_batch, dim3( (unsigned)((n + 255ul)/256ul) ), dim3( 256 ), 0, st, n, d_pool, d_off, d_sz,
                      d_hash );
  SH_CHECK( hipGetLastError() );
  return 0;
}

int
fd_shred_hip_roots_dev( fd_ed25519_hip_ctx_t * ctx, ulong n, uchar const * d_pool, uint const * d_off,
                        uint const * d_sz, uchar * d_roots, uchar * d_flags, void * stream ) {
  if( !n ) return 0;
  if( n > (ulong)UINT32_MAX ) return -1;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)fd_ed25519_hip_ctx_stream( ctx );
  SH_CHECK( hipSetDevice( fd_ed25519_hip_ctx_device( ctx ) ) );
  launch_roots( st, n, d_pool, d_off, d_sz, d_roots, d_flags );
  return 0;
}

fd_shred_hip_t *
fd_shred_hip_new( fd_ed25519_hip_ctx_t * ctx, ulong n_max ) {
  if( !ctx || !n_max || n_max > (1ul << 30) ) return 0;
  SH_CHECK( hipSetDevice( fd_ed25519_hip_ctx_device( ctx ) ) );
  fd_shred_hip_t * s = (fd_shred_hip_t *)calloc( 1, sizeof(fd_shred_hip_t) );
  if( !s ) return 0;
  ulong n = n_max, t = 64ul;
  while( t < 2ul*n ) t <<= 1;
  s->ctx = ctx; s->n_max = n; s->tsize = t;
  s->salt = (u32)std::random_device{}();
  fd_ed25519_hip_ctx_reserve( ctx, n );              /* one verify launch pair per call */
  SH_CHECK( hipMalloc( &s->d_tab, 4ul*t ) );       SH_CHECK( hipMalloc( &s->d_stat, 8 ) );
  SH_CHECK( hipMalloc( &s->d_rep, 4ul*n ) );       SH_CHECK( hipMalloc( &s->d_slot, 4ul*n ) );
  SH_CHECK( hipMalloc( &s->d_rroot, 32ul*n + 16ul ) );
  SH_CHECK( hipMalloc( &s->d_rsig, 64ul*n ) );     SH_CHECK( hipMalloc( &s->d_rpub, 32ul*n ) );
  SH_CHECK( hipMalloc( &s->d_rmoff, 4ul*n ) );     SH_CHECK( hipMalloc( &s->d_rmsz, 4ul*n ) );
  SH_CHECK( hipMalloc( &s->d_rcode, n ) );
  SH_CHECK( hipMemset( s->d_stat, 0, 8 ) );
  SH_CHECK( hipMemset( s->d_rroot, 0, 32ul*n + 16ul ) );
  SH_CHECK( hipEventCreateWithFlags( &s->ev_last, hipEventDisableTiming ) );
  return s;
}

void
fd_shred_hip_delete( fd_shred_hip_t * s ) {
  if( !s ) return;
  (void)hipSetDevice( fd_ed25519_hip_ctx_device( s->ctx ) );
  (void)hipStreamSynchronize( (hipStream_t)fd_ed25519_hip_ctx_stream( s->ctx ) );
  if( s->ev_used ) (void)hipEventSynchronize( s->ev_last );
  (void)hipEventDestroy( s->ev_last );
  (void)hipFree( s->d_tab ); (void)hipFree( s->d_stat ); (void)hipFree( s->d_rep ); (void)hipFree( s->d_slot );
  (void)hipFree( s->d_rroot ); (void)hipFree( s->d_rsig ); (void)hipFree( s->d_rpub ); (void)hipFree( s->d_rmoff );
  (void)hipFree( s->d_rmsz ); (void)hipFree( s->d_rcode );
  free( s );
}

int
fd_shred_hip_verify_dev( fd_shred_hip_t * s, ulong n, uchar const * d_pool, uint const * d_off, uint const * d_sz,
                         uchar const * d_pubs, uchar * d_roots, uchar * d_flags, signed char * d_codes,
                         void * stream ) {
  if( n > s->n_max ) return -1;
  if( !n ) return 0;
  hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)fd_ed25519_hip_ctx_stream( s->ctx );
  SH_CHECK( hipSetDevice( fd_ed25519_hip_ctx_device( s->ctx ) ) );
  dim3 grid( (unsigned)((n + 255ul)/256ul) ), blk( 256 );
  if( s->ev_used ) SH_CHECK( hipStreamWaitEvent( st, s->ev_last, 0 ) );   /* the scratch is the previous call's until then */
  SH_CHECK( hipMemsetAsync( s->d_tab, 0xff, 4ul*s->tsize, st ) );
  SH_CHECK( hipMemsetAsync( s->d_stat, 0, 8, st ) );
  launch_roots( st, n, d_pool, d_off, d_sz, d_roots, d_flags );
  hipLaunchKernelGGL( k_shred_pick, grid, blk, 0, st, n, d_pool, d_off, d_pubs, (uchar const *)d_roots,
                      (uchar const *)d_flags, s->d_tab, (u32)(s->tsize - 1ul), s->salt, s->d_stat, s->d_rep, s->d_slot,
                      s->d_rroot, s->d_rsig, s->d_rpub, s->d_rmoff, s->d_rmsz );
  SH_CHECK( hipGetLastError() );
  fd_ed25519_hip_verify_dev_count( s->ctx, n, s->d_stat, s->d_rsig, s->d_rpub, s->d_rroot, s->d_rmoff, s->d_rmsz,
                                   s->d_rcode, NULL, st );
  hipLaunchKernelGGL( k_shred_scatter, grid, blk, 0, st, n, (uchar const *)d_flags, (u32 const *)s->d_rep,
                      (u32 const *)s->d_slot, (signed char const *)s->d_rcode, d_codes );
  SH_CHECK( hipGetLastError() );
  SH_CHECK( hipEventRecord( s->ev_last, st ) );
  s->ev_used = 1;
  return 0;
}

void
fd_shred_hip_stats( fd_shred_hip_t const * s, ulong out[ 2 ] ) {
  u32 h[2] = { 0u, 0u };
  SH_CHECK( hipSetDevice( fd_ed25519_hip_ctx_device( s->ctx ) ) );
  SH_CHECK( hipMemcpy( h, s->d_stat, 8, hipMemcpyDeviceToHost ) );
  out[0] = h[1]; out[1] = h[0];
}

} /* extern "C" */
