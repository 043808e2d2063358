/* fd_sha256_dev.h -- device SHA-256 for gfx950 (fd_shred_hip.hip).

   The GPU counterpart of the reference's SHA-256 (src/ballet/sha256/
   fd_sha256.c) for the one shape the shred path needs: many messages of
   about a kilobyte, one per lane, each read once.  Same structure as the
   SHA-512 of the verify path (fd_ed25519_dev.h sha512_prefixed_coop): the
   compression runs in registers, the message blocks reach the lanes through
   LDS, loaded by the whole wave in 16-byte pieces. */

#pragma once
#include "fd_ed25519_dev.h"

static __device__ const u32 SHA256_K[64] = {
  0x428a2f98u,0x71374491u,0xb5c0fbcfu,0xe9b5dba5u,0x3956c25bu,0x59f111f1u,0x923f82a4u,0xab1c5ed5u,
  0xd807aa98u,0x12835b01u,0x243185beu,0x550c7dc3u,0x72be5d74u,0x80deb1feu,0x9bdc06a7u,0xc19bf174u,
  0xe49b69c1u,0xefbe4786u,0x0fc19dc6u,0x240ca1ccu,0x2de92c6fu,0x4a7484aau,0x5cb0a9dcu,0x76f988dau,
  0x983e5152u,0xa831c66du,0xb00327c8u,0xbf597fc7u,0xc6e00bf3u,0xd5a79147u,0x06ca6351u,0x14292967u,
  0x27b70a85u,0x2e1b2138u,0x4d2c6dfcu,0x53380d13u,0x650a7354u,0x766a0abbu,0x81c2c92eu,0x92722c85u,
  0xa2bfe8a1u,0xa81a664bu,0xc24b8b70u,0xc76c51a3u,0xd192e819u,0xd6990624u,0xf40e3585u,0x106aa070u,
  0x19a4c116u,0x1e376c08u,0x2748774cu,0x34b0bcb5u,0x391c0cb3u,0x4ed8aa4au,0x5b9cca4fu,0x682e6ff3u,
  0x748f82eeu,0x78a5636fu,0x84c87814u,0x8cc70208u,0x90befffau,0xa4506cebu,0xbef9a3f7u,0xc67178f2u };

DEV u32 rotr32( u32 x, u32 n ) { return __builtin_amdgcn_alignbit( x, x, n ); }

DEV void sha256_init( u32 st[8] ) {
  st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
  st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}

/* one compression; W holds the block's 16 big-endian words and is used as
   the rolling message schedule */
DEV void sha256_block( u32 st[8], u32 W[16] ) {
  u32 a=st[0], b=st[1], c=st[2], d=st[3], e=st[4], f=st[5], g=st[6], h=st[7];
  #pragma unroll
  for( int t=0; t<64; t++ ) {
    u32 w;
    if( t < 16 ) w = W[t];
    else {
      u32 w15 = W[(t+1)&15], w2 = W[(t+14)&15];
      u32 s0 = rotr32( w15, 7u ) ^ rotr32( w15, 18u ) ^ (w15 >> 3);
      u32 s1 = rotr32( w2, 17u ) ^ rotr32( w2, 19u ) ^ (w2 >> 10);
      w = W[t&15] + s0 + s1 + W[(t+9)&15];
      W[t&15] = w;
    }
    u32 t1 = h + (rotr32( e, 6u ) ^ rotr32( e, 11u ) ^ rotr32( e, 25u )) + (g ^ (e & (f ^ g))) + SHA256_K[t] + w;
    u32 t2 = (rotr32( a, 2u ) ^ rotr32( a, 13u ) ^ rotr32( a, 22u )) + ((a & b) | (c & (a | b)));
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  st[0]+=a; st[1]+=b; st[2]+=c; st[3]+=d; st[4]+=e; st[5]+=f; st[6]+=g; st[7]+=h;
}

/* ---- SHA-256( prefix || M ) with LDS-staged, wave-cooperative blocks -------

   For all 64 lanes of a wave at once (wave-uniform control flow: every lane
   calls it; a lane with nothing to hash passes on = false and gets no
   digest).  PLEN is 0 (plain SHA-256) or 26 (the bmtree's long prefixes,
   fd_bmtree.c:52-142), pre the prefix as 7 little-endian words (bytes 26, 27
   zero).

   The hashed stream is laid over memory at v = msg - PLEN, so that block b
   is always the 64 bytes at v + 64 b, whatever the prefix length: the
   prefix's own bytes are put in after the load, in registers (block 0
   only).  For PLEN = 26 the caller therefore guarantees that the 41 bytes
   before msg are readable (for a shred msg = shred + 64: its signature).
   Per block, up to the wave's largest block count:
     1. each lane publishes its window -- the 16-byte-aligned base of
        v + 64 b and the number of 16-byte chunks (<= 5) that cover the
        window's bytes up to the end of the message -- in LDS;
     2. the wave loads the 64 windows together: piece p = lane + 64 i (i < 5)
        is chunk p % 5 of lane p / 5's window, so 5 neighbouring lanes read
        one message's 80 bytes as contiguous 16-byte loads instead of 64
        lanes each walking a message 1.2 KB from the next;
     3. each lane reads its 17 words back at its own byte offset, shifts them
        into place (alignbit), zeroes what lies past the message and sets
        the 0x80 pad (chunks past the message are never loaded: what LDS
        still holds there is masked off here), and compresses.
   buf: this wave's 64 x SHA256_WIN_WORDS words of LDS, 16-byte aligned;
   meta: its 64 u64.  Memory must be readable up to the 16-byte boundary
   after each message's last byte.  A lane's 20-word stride makes the 17
   read-backs 4-way bank conflicts; the compression's ~2000 VALU operations
   per block hide them. */
#define SHA256_WIN_WORDS 20u

template<u32 PLEN>
DEV void sha256_coop( u32 st[8], u32 const * pre, u8 const * msg, u32 msz, bool on, u32 * buf, u64 * meta, u32 lane ) {
  sha256_init( st );
  u32 tot = PLEN + msz;
  u32 nb = on ? (tot + 9u + 63u) >> 6 : 0u;
  u32 nbmax = wave_max_u32( nb );
  u8 const * v = msg - PLEN;
  u32 const * own = buf + SHA256_WIN_WORDS*lane;
  #pragma unroll 1
  for( u32 b=0; b<nbmax; b++ ) {
    bool act = b < nb;
    u32 lo = 64u*b;
    u32 hi = min( tot, lo + 64u );
    u32 nbytes = (act && hi > lo) ? hi - lo : 0u;
    uintptr_t addr = (uintptr_t)(v + lo);
    u32 o = (u32)(addr & 15u);
    u32 nch = nbytes ? (o + nbytes + 15u) >> 4 : 0u;
    meta[lane] = ((u64)(addr >> 4) & 0xfffffffffffULL) | ((u64)nch << 44);
    wave_lds_sync();
    #pragma unroll
    for( u32 i=0; i<5u; i++ ) {                           /* 320 pieces = 64 windows x 5 chunks */
      u32 pc = lane + 64u*i, r = pc / 5u, c = pc - 5u*r;
      u64 mr = meta[r];
      if( c < (u32)(mr >> 44) )
        ((uint4 *)(buf + SHA256_WIN_WORDS*r))[c] = ((uint4 const *)(uintptr_t)((mr & 0xfffffffffffULL) << 4))[c];
    }
    wave_lds_sync();
    u32 mw[17];
    u32 const * rp = own + (o >> 2);
    #pragma unroll
    for( int k=0; k<17; k++ ) mw[k] = rp[k];
    u32 sh = (o & 3u) * 8u;
    u32 W[16];                                            /* stream bytes [lo + 4k, +4), little-endian */
    #pragma unroll
    for( int k=0; k<16; k++ ) W[k] = __builtin_amdgcn_alignbit( mw[k+1], mw[k], sh );
    if( PLEN && b == 0u ) {                               /* wave-uniform */
      #pragma unroll
      for( int k=0; k<6; k++ ) W[k] = pre[k];
      W[6] = (W[6] & 0xffff0000u) | pre[6];
    }
    int e = (int)tot - (int)lo;                           /* the message ends at byte e of this block */
    if( e < 64 ) {
      #pragma unroll
      for( int k=0; k<16; k++ ) {
        int rel = e - 4*k;                                /* bytes of word k before the pad */
        u32 keep = rel >= 4 ? ~0u : rel <= 0 ? 0u : (1u << (8*rel)) - 1u;
        u32 pad = (rel >= 0 && rel < 4) ? 0x80u << (8*rel) : 0u;
        W[k] = (W[k] & keep) | pad;
      }
    }
    #pragma unroll
    for( int k=0; k<16; k++ ) W[k] = bswap32( W[k] );
    if( b + 1u == nb ) { W[14] = tot >> 29; W[15] = tot << 3; }
    if( act ) sha256_block( st, W );
    wave_lds_sync();                                      /* the next block reuses the buffers */
  }
}

/* SHA-256( pre(26) || L[0,20) || R[0,20) ): the bmtree's branch node of two
   20-byte-truncated children (fd_bmtree.c:95-142), 66 bytes in two blocks,
   all in registers.  L and R are the children's first five little-endian
   words; st gets the digest's state words. */
DEV void sha256_merge20( u32 st[8], u32 const * pre, u32 const L[5], u32 const R[5] ) {
  u32 m[17];                                              /* the 66 bytes and the pad, little-endian words */
  #pragma unroll
  for( int k=0; k<6; k++ ) m[k] = pre[k];
  m[6] = pre[6] | (L[0] << 16);
  #pragma unroll
  for( int k=1; k<5; k++ ) m[6+k] = (L[k-1] >> 16) | (L[k] << 16);
  m[11] = (L[4] >> 16) | (R[0] << 16);
  #pragma unroll
  for( int k=1; k<5; k++ ) m[11+k] = (R[k-1] >> 16) | (R[k] << 16);
  m[16] = (R[4] >> 16) | 0x00800000u;
  sha256_init( st );
  #pragma unroll 1
  for( u32 blk=0; blk<2u; blk++ ) {                       /* one copy of the compression's code */
    u32 W[16];
    #pragma unroll
    for( int k=0; k<16; k++ ) W[k] = blk ? (k == 0 ? bswap32( m[16] ) : k == 15 ? 66u*8u : 0u) : bswap32( m[k] );
    sha256_block( st, W );
  }
}
