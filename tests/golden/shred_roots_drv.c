/* shred_roots_drv.c -- expected Merkle roots for tests/golden/shred_roots.npz
   (built and run by tests/golden/gen_shred_roots.py against the reference's
   sources; calls only the reference's public functions).

     shred_roots_drv <in.bin> <out.bin>

   in:   uint n, then n x { uint sz, uchar shred[1228] } synthetic shreds
   out:  n x { uchar ok, uchar root[32] }: ok = fd_shred_parse accepted the
         shred and fd_shred_merkle_root returned success
         uchar leader[32]
         2 x 64 x { uint sz, uchar shred[1228], uchar ok, uchar root[32] }:
         two FEC sets of 32 data and 32 code shreds cut by fd_shredder (as
         integration/fec_run.c drives it) from fixed pseudo-random batches,
         the first unchained, the second chained and (as its block's last set)
         resigned, signed by a fixed key */

#include "../../util/fd_util.h"
#include "../../ballet/shred/fd_shred.h"
#include "../../ballet/bmtree/fd_bmtree.h"
#include "../../ballet/ed25519/fd_ed25519.h"
#include "fd_shredder.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK( c ) do { if( !(c) ) { fprintf( stderr, "shred_roots_drv: %s failed (line %d)\n", #c, __LINE__ ); exit( 1 ); } } while(0)

typedef struct { fd_sha512_t sha[1]; uchar const * prv; uchar const * pub; } signer_t;

static void
sign_root( void * _s, uchar * sig, uchar const * root ) {
  signer_t * s = (signer_t *)_s;
  fd_ed25519_sign( sig, root, 32UL, s->pub, s->prv, s->sha );
}

static uchar bmtree_mem[ FD_BMTREE_COMMIT_FOOTPRINT( FD_SHRED_MERKLE_LAYER_CNT ) ] __attribute__((aligned(FD_BMTREE_COMMIT_ALIGN)));

static void
put_root( FILE * out, uchar const * buf, ulong sz ) {
  fd_bmtree_node_t root[1];
  memset( root, 0, sizeof(root) );
  fd_shred_t const * shred = fd_shred_parse( buf, sz );
  uchar ok = (uchar)( shred && fd_shred_merkle_root( shred, bmtree_mem, root ) );
  CHECK( fwrite( &ok, 1UL, 1UL, out )==1UL && fwrite( root->hash, 1UL, 32UL, out )==32UL );
}

int
main( int argc, char ** argv ) {
  CHECK( argc==3 );
  FILE * in  = fopen( argv[1], "rb" ); CHECK( in );
  FILE * out = fopen( argv[2], "wb" ); CHECK( out );

  uint n;
  CHECK( fread( &n, 4UL, 1UL, in )==1UL );
  for( uint i=0U; i<n; i++ ) {
    uint sz; uchar buf[ FD_SHRED_MAX_SZ ];
    CHECK( fread( &sz, 4UL, 1UL, in )==1UL && fread( buf, 1UL, FD_SHRED_MAX_SZ, in )==FD_SHRED_MAX_SZ );
    CHECK( sz<=FD_SHRED_MAX_SZ );
    put_root( out, buf, sz );
  }
  fclose( in );

  fd_rng_t _rng[1]; fd_rng_t * rng = fd_rng_join( fd_rng_new( _rng, 0x5eed5eedU, 7UL ) );
  uchar prv[ 32 ], pub[ 32 ];
  fd_sha512_t sha[1]; CHECK( fd_sha512_join( fd_sha512_new( sha ) ) );
  for( ulong b=0UL; b<32UL; b++ ) prv[ b ] = fd_rng_uchar( rng );
  CHECK( fd_ed25519_public_from_private( pub, prv, sha ) );
  CHECK( fwrite( pub, 1UL, 32UL, out )==32UL );
  signer_t sg[1];
  CHECK( fd_sha512_join( fd_sha512_new( sg->sha ) ) );
  sg->prv = prv; sg->pub = pub;
  static fd_shredder_t shredder_mem[1];
  fd_shredder_t * sh = fd_shredder_join( fd_shredder_new( shredder_mem, sign_root, sg ) );
  CHECK( sh );
  fd_shredder_set_shred_version( sh, (ushort)6051 );

  static uchar tmp[ 2048UL*(FD_REEDSOL_DATA_SHREDS_MAX+FD_REEDSOL_PARITY_SHREDS_MAX) ];
  static uchar batch[ FD_SHREDDER_NORMAL_FEC_SET_PAYLOAD_SZ ];
  fd_fec_set_t set_mem[1];
  uchar * p = tmp;
  for( ulong j=0UL; j<FD_REEDSOL_DATA_SHREDS_MAX;   j++ ) { set_mem->data_shreds  [ j ] = p; p += 2048UL; }
  for( ulong j=0UL; j<FD_REEDSOL_PARITY_SHREDS_MAX; j++ ) { set_mem->parity_shreds[ j ] = p; p += 2048UL; }
  uchar chained[ 32 ];
  for( ulong b=0UL; b<32UL; b++ ) chained[ b ] = fd_rng_uchar( rng );

  for( ulong k=0UL; k<2UL; k++ ) {
    ulong bsz = k ? FD_SHREDDER_RESIGNED_FEC_SET_PAYLOAD_SZ : FD_SHREDDER_NORMAL_FEC_SET_PAYLOAD_SZ;   /* 32 data shreds each */
    for( ulong b=0UL; b<bsz; b++ ) batch[ b ] = fd_rng_uchar( rng );
    fd_entry_batch_meta_t meta[1]; memset( meta, 0, sizeof(meta) ); meta->block_complete = 1; meta->parent_offset = 1UL;
    CHECK( fd_shredder_init_batch( sh, batch, bsz, 1UL+k, meta ) );
    fd_fec_set_t * set = fd_shredder_next_fec_set( sh, set_mem, k ? chained : NULL, NULL );
    CHECK( set );
    if( set->data_shred_cnt!=32UL || set->parity_shred_cnt!=32UL ) {
      fprintf( stderr, "shred_roots_drv: set %lu has %lu data + %lu code shreds\n", k, set->data_shred_cnt, set->parity_shred_cnt );
      exit( 1 );
    }
    for( ulong j=0UL; j<64UL; j++ ) {
      uchar buf[ FD_SHRED_MAX_SZ ];
      uint  sz = j<32UL ? (uint)FD_SHRED_MIN_SZ : (uint)FD_SHRED_MAX_SZ;
      memset( buf, 0, sizeof(buf) );
      memcpy( buf, j<32UL ? set->data_shreds[ j ] : set->parity_shreds[ j-32UL ], sz );
      CHECK( fwrite( &sz, 4UL, 1UL, out )==1UL && fwrite( buf, 1UL, FD_SHRED_MAX_SZ, out )==FD_SHRED_MAX_SZ );
      put_root( out, buf, sz );
    }
    CHECK( fd_shredder_fini_batch( sh ) );
  }
  CHECK( !fclose( out ) );
  return 0;
}
