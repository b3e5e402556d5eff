// INT4 cross-attention caches (wh_context_create_kv4): the quantizer behind the encoder's cross-K/V product and the decode step's cross-attention over the
// nibble caches, every multiply-add of it on v_mfma_i32_32x32x32_i8 (DESIGN.md section 7 "INT4 cross-attention caches"; tests/cross_i4_ref.py pins the format).
//
// Format. Per key row of 64 FP16 values: s = amax / 7 (IEEE FP32 division; 1 for a row of zeros), n = rint( x / s ) (IEEE FP32 division, to nearest even)
// clamped to [-7, 7] -- the rule of the INT8 encoder rows (quant_i8.hip) with 7 for 127 -- stored as the nibble n + 8: 1 .. 15, never 0. One FP32 scale per key
// row, [layer][window][head][T], K and V apart.
//   K  [layer][window][head][T][32 bytes]: byte t of a row holds dim 2 t in its low nibble and dim 2 t + 1 in its high nibble.
//   V  [layer][window][head][ceil( T / 64 )][64 dims][32 bytes]: blocks of 64 keys, dim-major inside a block; the 32 bytes of a dim are 8 words of 8 keys, byte t
//      of word w holding key 8 w + t in its low nibble and key 8 w + 4 + t in its high nibble. Keys behind T inside the last block are written as nibble 0.
// Both orders are the ones ( w & 0x0F0F0F0F, ( w >> 4 ) & 0x0F0F0F0F ) leaves in the matrix instruction's k order without a permute: for K the query is laid out
// to match (once per launch), for V the softmax weights of consecutive keys are consecutive bytes.
//
// attentionDecG4. Grid (head, window group, token), 512 threads; wave w owns keys 192 w .. 192 w + 191 in every phase.
//   loads    lane l owns bytes 16 ( l >> 5 ) .. + 15 of key row l & 31 of a 32-key block: a wave instruction reads 32 whole rows = 1 KiB contiguous; the 6 loads of a
//            thread (and its 6 K scales) are requested before LayerNorm and the query projection. The 6 V loads (a 64-key block x 32 dims each, 1 KiB contiguous)
//            go out behind the last score instruction and land under the softmax.
//   unpack   three vector instructions per word of eight nibbles; the +8 of the codes is taken out once per query: 8 * ( sum of the query's term ).
//   scores   D = A B with the QUERY TERMS as the 32 rows of A and 32 keys as the columns of B (a lane's 16 accumulators are then the terms of NQ / 2 queries for
//            ONE key: the terms are combined inside the lane, no shuffle). q = sq ( a + b / 256 + c / 65536 ) with sq a power of two per (row, head) and a, b, c
//            balanced int8 digits of rint( 65536 q / sq ): row 4 q + term, a fourth row of zeros. Two instructions (dims 0..31 | 32..63 come in the two lane halves,
//            the two words pairs of a load in the two instructions) give 32 keys x all queries.
//   softmax  attentionDecG's: scores in LDS, maximum over all keys, exp16, double sum.
//   P.V      the same instruction: rows of A are the terms of p = e * scaleV[ key ] relative to a power of two sp >= max p / 127 of the wave's 192 keys, columns of B
//            32 dims, the K depth 32 keys; int32 accumulation over the wave's keys is exact, the three term rows, the -8 sum( p ) of the code offset and sp are
//            combined once per wave in FP64 (exact), the eight waves' FP32 partial rows are added through LDS and divided by the double sum.
// Padding: rows behind nKeys are never loaded for K (clamped), their V nibbles meet zero terms in an integer product, their scales are never read.
#include "kernels.h"

namespace wh
{
	namespace
	{
		typedef __attribute__( ( ext_vector_type( 4 ) ) ) int i32x4;
		typedef __attribute__( ( ext_vector_type( 16 ) ) ) int i32x16;

		constexpr int MAX_KEYS = 1536;
		constexpr int NT = 512;
		constexpr int NW = NT / 64;
		constexpr int G4_MAXD = 1280;
		constexpr int G4_WKEYS = MAX_KEYS / NW;		// keys of a wave (192)
		constexpr int G4_KIT = G4_WKEYS / 32;		// K loads of a thread: 32-key blocks of the wave (6)
		constexpr int G4_VIT = G4_WKEYS / 64;		// 64-key V blocks of the wave (3), two loads each (dims 0..31, 32..63)
		constexpr int V4_BLOCK = 64 * 32;			// bytes of a V block: 64 dims x 64 keys
		constexpr unsigned NIB = 0x0F0F0F0Fu;

		__device__ __forceinline__ int waveReduceSumI( int v )
		{
#pragma unroll
			for( int o = 32; o > 0; o >>= 1 ) v += __shfl_xor( v, o, 64 );
			return v;
		}

		// ---------------------------------------------------------------------------------------------------------------
		// quantizeCrossKV4: a 256-thread workgroup takes 64 keys of one (window, head) and one set (blockIdx.z: K, V). Four lanes own a 128-byte FP16 row (two 16-byte
		// loads each), the row's amax by two xor-shuffles. K: a lane's 16 codes are 8 bytes; lane pairs exchange them and the even lane stores 16. V: the codes go
		// through LDS as bytes [key][dim] and 128 threads each gather the 32 keys of one (dim, half) into one 16-byte store: the block leaves as 2 KiB contiguous.
		// ---------------------------------------------------------------------------------------------------------------
		constexpr int Q4_NT = 256;
		struct Quant4Args
		{
			const f16* src[ 2 ];
			uint8_t* dst[ 2 ];
			float* scale[ 2 ];
			int T;
		};

		__device__ __forceinline__ float rowScaleI4( float amax ) { return amax > 0.0f ? __fdiv_rn( amax, 7.0f ) : 1.0f; }
		__device__ __forceinline__ unsigned quantOneI4( f16 x, float s )
		{
			const float r = fminf( fmaxf( rintf( __fdiv_rn( (float)x, s ) ), -7.0f ), 7.0f );
			return (unsigned)( (int)r + 8 );
		}

		__global__ void __launch_bounds__( Q4_NT ) quantizeCrossKV4( const Quant4Args a )
		{
			__shared__ __attribute__( ( aligned( 16 ) ) ) uint8_t cod[ 64 ][ HEAD_DIM ];
			const int set = blockIdx.z;
			if( !a.dst[ set ] ) return;
			const int tid = threadIdx.x, kl = tid >> 2, c = tid & 3;
			const int kb = blockIdx.x, nkb = gridDim.x;
			const long long head = blockIdx.y;
			const int key = kb * 64 + kl;
			const long long row = head * a.T + ( key < a.T ? key : a.T - 1 );
			const f16* const src = a.src[ set ] + row * HEAD_DIM + c * 16;
			const f16x8 x0 = __builtin_nontemporal_load( (const f16x8*)src );
			const f16x8 x1 = __builtin_nontemporal_load( (const f16x8*)( src + 8 ) );
			float amax = 0.0f;
#pragma unroll
			for( int e = 0; e < 8; e++ ) amax = fmaxf( amax, fmaxf( fabsf( (float)x0[ e ] ), fabsf( (float)x1[ e ] ) ) );
			amax = fmaxf( amax, __shfl_xor( amax, 1, 64 ) );
			amax = fmaxf( amax, __shfl_xor( amax, 2, 64 ) );
			const float s = rowScaleI4( amax );
			unsigned n[ 16 ];
#pragma unroll
			for( int e = 0; e < 8; e++ )
			{
				n[ e ] = quantOneI4( x0[ e ], s );
				n[ 8 + e ] = quantOneI4( x1[ e ], s );
			}
			if( key < a.T && c == 0 ) a.scale[ set ][ row ] = s;
			if( set == 0 )
			{
				unsigned w0 = 0u, w1 = 0u;
#pragma unroll
				for( int t = 0; t < 4; t++ )
				{
					w0 |= ( n[ 2 * t ] | ( n[ 2 * t + 1 ] << 4 ) ) << ( 8 * t );
					w1 |= ( n[ 8 + 2 * t ] | ( n[ 9 + 2 * t ] << 4 ) ) << ( 8 * t );
				}
				const unsigned p0 = __shfl_xor( w0, 1, 64 ), p1 = __shfl_xor( w1, 1, 64 );
				if( key < a.T && ( c & 1 ) == 0 ) *(u32x4*)( a.dst[ 0 ] + row * 32 + c * 8 ) = u32x4{ w0, w1, p0, p1 };
				return;
			}
			u32x4 b = { 0u, 0u, 0u, 0u };
			if( key < a.T )
#pragma unroll
				for( int e = 0; e < 16; e++ ) b[ e >> 2 ] |= n[ e ] << ( 8 * ( e & 3 ) );
			*(u32x4*)( &cod[ kl ][ c * 16 ] ) = b;
			__syncthreads();
			if( tid < 128 )
			{
				const int dim = tid >> 1, g = tid & 1;
				u32x4 o;
#pragma unroll
				for( int w = 0; w < 4; w++ )
				{
					unsigned v = 0u;
#pragma unroll
					for( int t = 0; t < 4; t++ )
						v |= ( (unsigned)cod[ 32 * g + 8 * w + t ][ dim ] | ( (unsigned)cod[ 32 * g + 8 * w + 4 + t ][ dim ] << 4 ) ) << ( 8 * t );
					o[ w ] = v;
				}
				*(u32x4*)( a.dst[ 1 ] + ( head * nkb + kb ) * V4_BLOCK + dim * 32 + g * 16 ) = o;
			}
		}

		// ---------------------------------------------------------------------------------------------------------------
		// attentionDecG4
		// ---------------------------------------------------------------------------------------------------------------
		template<int NQ>
		struct DecG4Lds
		{
			float sc[ NQ ][ MAX_KEYS ];
			float qs[ NQ ][ HEAD_DIM ];
			float red[ NQ ][ NW ][ HEAD_DIM ];
			float shf[ NQ ][ NW ];
			double shd[ NQ ][ NW ];
			float sq[ NQ ];				// the query's power-of-two scale
			int qcorr[ NQ ][ 4 ];		// 8 * ( sum of the query's term over the 64 dims ): the +8 of the K codes
			__attribute__( ( aligned( 16 ) ) ) int8_t qt[ NQ ][ 3 ][ HEAD_DIM ];			 // the query's terms in the k order the unpacked K words have
			__attribute__( ( aligned( 16 ) ) ) int8_t pt[ NW ][ NQ ][ 3 ][ G4_WKEYS ];	 // the terms of p for the wave's keys
			__attribute__( ( aligned( 16 ) ) ) f16 xn[ NQ ][ G4_MAXD ];
		};

		__device__ __forceinline__ float xorReduce8( float v )
		{
			v += __shfl_xor( v, 1, 64 );
			v += __shfl_xor( v, 2, 64 );
			v += __shfl_xor( v, 4, 64 );
			return v;
		}

		template<bool NT_LOADS>
		__device__ __forceinline__ u32x4 loadRow16( const uint8_t* p )
		{
			if constexpr( NT_LOADS ) return __builtin_nontemporal_load( (const u32x4*)p );
			else return *(const u32x4*)p;
		}

		// two words of eight nibbles -> 16 bytes 0 .. 15: [ low nibbles of w0 | high nibbles of w0 | low of w1 | high of w1 ]
		__device__ __forceinline__ i32x4 unpackNibbles( unsigned w0, unsigned w1 )
		{
			return i32x4{ (int)( w0 & NIB ), (int)( ( w0 >> 4 ) & NIB ), (int)( w1 & NIB ), (int)( ( w1 >> 4 ) & NIB ) };
		}

		// The power of two s with 127 s >= amax > 0, and 65536 / s: 127 = 1.984375 * 2^6. amax below 2^-100 counts as zero (s = 1: every term is 0).
		__device__ __forceinline__ void termScale( float amax, float& s, float& inv16 )
		{
			if( !( amax >= 7.9e-31f ) ) { s = 1.0f; inv16 = 65536.0f; return; }
			const unsigned bits = __builtin_bit_cast( unsigned, amax );
			const int e = (int)( bits >> 23 ) - 127 - 6 + ( ( bits & 0x7fffffu ) > 0x7E0000u ? 1 : 0 );
			s = __builtin_bit_cast( float, (unsigned)( e + 127 ) << 23 );
			inv16 = __builtin_bit_cast( float, (unsigned)( 127 + 16 - e ) << 23 );
		}

		// X = 65536 a + 256 b + c with a, b, c in [-128, 127] (balanced digits; |X| <= 127 * 65536 keeps a in [-127, 127])
		__device__ __forceinline__ void splitTerms( int X, int& a, int& b, int& c )
		{
			c = (int)(int8_t)X;
			const int X1 = ( X - c ) >> 8;
			b = (int)(int8_t)X1;
			a = ( X1 - b ) >> 8;
		}

		template<int NQ, bool FUSEQ, bool NT_LOADS = false>
		__global__ void __launch_bounds__( NT, NQ == 1 ? 4 : 2 ) attentionDecG4( const DecAttnArgs a )
		{
			extern __shared__ __attribute__( ( aligned( 16 ) ) ) unsigned char smemG4[];
			DecG4Lds<NQ>& L = *(DecG4Lds<NQ>*)smemG4;
			constexpr int NQ2 = ( NQ + 1 ) / 2;	  // queries a lane half sees in its accumulators: q = 2 qq + ( lane >> 5 )

			const int tid = threadIdx.x;
			const int lane = tid & 63;
			const int wave = tid >> 6;
			const int j32 = lane & 31, g = lane >> 5;
			const int h = blockIdx.x, bw = blockIdx.y, i = blockIdx.z;
			const int d = a.H * HEAD_DIM;
			const long long head = ( (long long)bw * a.H + h ) * a.keyStride;
			const int vBlocks = ( a.keyStride + 63 ) >> 6;
			const uint8_t* const K = a.kc4 + head * 32 + g * 16;
			const uint8_t* const V = a.vc4 + ( (long long)bw * a.H + h ) * vBlocks * V4_BLOCK + j32 * 32 + g * 16;
			const float* const KS = a.kScale + head;
			const float* const VS = a.vScale + head;
			const int nk = a.nKeys;
			const int lastRow = nk - 1;
			const int key0 = wave * G4_WKEYS;
			auto rowOf = [ & ]( int q ) -> long long { return ( (long long)bw * NQ + q ) * a.nTok + i; };

			// ---- every K row of this thread goes out before anything else (rows beyond nk are clamped), with the scales of the same keys ----
			u32x4 kr[ G4_KIT ];
			float ksr[ G4_KIT ];
#pragma unroll
			for( int u = 0; u < G4_KIT; u++ )
			{
				const int key = min( key0 + u * 32 + j32, lastRow );
				kr[ u ] = loadRow16<NT_LOADS>( K + (long long)key * 32 );
				ksr[ u ] = KS[ key ];
			}

			// ---- query: attentionDecG's, statement for statement ----
			if constexpr( FUSEQ )
			{
				const int nv = d >> 2;
				f32x4 xv[ NQ ];
				f32x4 wv = { 0, 0, 0, 0 }, bv = { 0, 0, 0, 0 };
				const bool own = tid < nv;
				if( own )
				{
					wv = *(const f32x4*)( a.lnW + tid * 4 );
					bv = *(const f32x4*)( a.lnB + tid * 4 );
				}
#pragma unroll
				for( int q = 0; q < NQ; q++ )
					xv[ q ] = own ? *(const f32x4*)( a.lnX + rowOf( q ) * d + tid * 4 ) : f32x4{ 0, 0, 0, 0 };
				const float invD = 1.0f / (float)d;
				float s[ NQ ];
#pragma unroll
				for( int q = 0; q < NQ; q++ ) s[ q ] = waveReduceSum( ( xv[ q ][ 0 ] + xv[ q ][ 1 ] ) + ( xv[ q ][ 2 ] + xv[ q ][ 3 ] ) );
				if( lane == 0 )
#pragma unroll
					for( int q = 0; q < NQ; q++ ) L.shf[ q ][ wave ] = s[ q ];
				__syncthreads();
				float mean[ NQ ];
#pragma unroll
				for( int q = 0; q < NQ; q++ )
				{
					float t = L.shf[ q ][ 0 ];
#pragma unroll
					for( int w = 1; w < NW; w++ ) t += L.shf[ q ][ w ];
					mean[ q ] = t * invD;
				}
				__syncthreads();
#pragma unroll
				for( int q = 0; q < NQ; q++ )
				{
					float t = 0.0f;
					if( own )
					{
#pragma unroll
						for( int e = 0; e < 4; e++ )
						{
							xv[ q ][ e ] -= mean[ q ];
							t = fmaf( xv[ q ][ e ], xv[ q ][ e ], t );
						}
					}
					s[ q ] = waveReduceSum( t );
				}
				if( lane == 0 )
#pragma unroll
					for( int q = 0; q < NQ; q++ ) L.shf[ q ][ wave ] = s[ q ];
				__syncthreads();
#pragma unroll
				for( int q = 0; q < NQ; q++ )
				{
					float t = L.shf[ q ][ 0 ];
#pragma unroll
					for( int w = 1; w < NW; w++ ) t += L.shf[ q ][ w ];
					const float rstd = 1.0f / sqrtf( t * invD + 1e-5f );
					if( own )
					{
						f16x4 hv;
#pragma unroll
						for( int e = 0; e < 4; e++ ) hv[ e ] = (f16)__fadd_rn( __fmul_rn( __fmul_rn( xv[ q ][ e ], rstd ), wv[ e ] ), bv[ e ] );
						*(f16x4*)( &L.xn[ q ][ tid * 4 ] ) = hv;
					}
				}
				__syncthreads();
				const int gw = tid >> 3, cw = tid & 7;
				const f16* const wr = a.qW + ( (long long)h * HEAD_DIM + gw ) * d + cw * 8;
				float acc[ NQ ];
#pragma unroll
				for( int q = 0; q < NQ; q++ ) acc[ q ] = 0.0f;
				const int steps = d >> 6;
				for( int s0 = 0; s0 < steps; s0 += 4 )
				{
					f16x8 wq[ 4 ];
#pragma unroll
					for( int u = 0; u < 4; u++ )
						if( s0 + u < steps ) wq[ u ] = *(const f16x8*)( wr + ( s0 + u ) * 64 );
#pragma unroll
					for( int u = 0; u < 4; u++ )
						if( s0 + u < steps )
						{
#pragma unroll
							for( int q = 0; q < NQ; q++ )
							{
								const f16x8 xq = *(const f16x8*)( &L.xn[ q ][ ( s0 + u ) * 64 + cw * 8 ] );
#pragma unroll
								for( int e = 0; e < 8; e++ ) acc[ q ] = fmaf( (float)wq[ u ][ e ], (float)xq[ e ], acc[ q ] );
							}
						}
				}
#pragma unroll
				for( int q = 0; q < NQ; q++ )
				{
					const float t = xorReduce8( acc[ q ] );
					if( cw == 0 ) L.qs[ q ][ gw ] = round16( ( t + a.qB[ h * HEAD_DIM + gw ] ) * a.qScale );
				}
			}
			else
			{
				if( tid < HEAD_DIM * NQ )
				{
					const int q = tid / HEAD_DIM, j = tid - q * HEAD_DIM;
					L.qs[ q ][ j ] = (float)a.q[ rowOf( q ) * d + h * HEAD_DIM + j ];
				}
			}
			__syncthreads();

			// ---- the query's int8 terms: wave q splits query q, lane = dim; the byte position is the k slot the unpacked K words give that dim ----
			if( wave < NQ )
			{
				const float v = L.qs[ wave ][ lane ];
				float sq, inv16;
				termScale( waveReduceMax( fabsf( v ) ), sq, inv16 );
				int t[ 3 ];
				splitTerms( (int)rintf( v * inv16 ), t[ 0 ], t[ 1 ], t[ 2 ] );
				const int pos = ( lane & ~7 ) + ( ( lane & 1 ) << 2 ) + ( ( lane & 7 ) >> 1 );
#pragma unroll
				for( int e = 0; e < 3; e++ )
				{
					L.qt[ wave ][ e ][ pos ] = (int8_t)t[ e ];
					const int sum = waveReduceSumI( t[ e ] );
					if( lane == 0 ) L.qcorr[ wave ][ e ] = 8 * sum;
				}
				if( lane == 0 ) L.sq[ wave ] = sq;
			}
			__syncthreads();

			// A operands of the score instructions: row j32 = 4 q + term; the two k halves of this lane half
			const int rq = j32 >> 2, term = j32 & 3;
			const bool rowUsed = term < 3 && rq < NQ;
			i32x4 qa0 = { 0, 0, 0, 0 }, qa1 = { 0, 0, 0, 0 };
			if( rowUsed )
			{
				qa0 = *(const i32x4*)( &L.qt[ rq ][ term ][ 32 * g ] );
				qa1 = *(const i32x4*)( &L.qt[ rq ][ term ][ 32 * g + 16 ] );
			}
			int corr[ NQ2 ][ 3 ];
			float sqq[ NQ2 ];
#pragma unroll
			for( int qq = 0; qq < NQ2; qq++ )
			{
				const int q = min( 2 * qq + g, NQ - 1 );
				sqq[ qq ] = L.sq[ q ];
#pragma unroll
				for( int e = 0; e < 3; e++ ) corr[ qq ][ e ] = L.qcorr[ q ][ e ];
			}

			// ---- scores: lane (j32, g) leaves the block's key j32 with the terms of queries 2 qq + g in accumulators 4 qq .. 4 qq + 2 ----
			float mxl[ NQ2 ];
#pragma unroll
			for( int qq = 0; qq < NQ2; qq++ ) mxl[ qq ] = -INFINITY;
#pragma unroll
			for( int u = 0; u < G4_KIT; u++ )
			{
				if( key0 + u * 32 >= nk ) continue;	  // wave-uniform
				i32x16 acc = {};
				acc = __builtin_amdgcn_mfma_i32_32x32x32_i8( qa0, unpackNibbles( kr[ u ][ 0 ], kr[ u ][ 1 ] ), acc, 0, 0, 0 );
				acc = __builtin_amdgcn_mfma_i32_32x32x32_i8( qa1, unpackNibbles( kr[ u ][ 2 ], kr[ u ][ 3 ] ), acc, 0, 0, 0 );
				const int key = key0 + u * 32 + j32;
#pragma unroll
				for( int qq = 0; qq < NQ2; qq++ )
				{
					const int q = 2 * qq + g;
					float sd = (float)( acc[ 4 * qq ] - corr[ qq ][ 0 ] );
					sd = fmaf( (float)( acc[ 4 * qq + 1 ] - corr[ qq ][ 1 ] ), 0x1p-8f, sd );
					sd = fmaf( (float)( acc[ 4 * qq + 2 ] - corr[ qq ][ 2 ] ), 0x1p-16f, sd );
					const float s = sd * ( sqq[ qq ] * ksr[ u ] );
					if( key < nk && q < NQ )
					{
						mxl[ qq ] = fmaxf( mxl[ qq ], s );
						L.sc[ q ][ key ] = s;
					}
				}
			}

			// the V blocks of this wave go out now: they do not depend on the softmax; so do the V scales of the keys this lane owns in the softmax pass
			u32x4 vr[ G4_VIT ][ 2 ];
#pragma unroll
			for( int kb = 0; kb < G4_VIT; kb++ )
			{
				const int blk = min( ( key0 >> 6 ) + kb, lastRow >> 6 );
#pragma unroll
				for( int dh = 0; dh < 2; dh++ ) vr[ kb ][ dh ] = loadRow16<NT_LOADS>( V + (long long)blk * V4_BLOCK + dh * 1024 );
			}
			float vsr[ G4_VIT ];
#pragma unroll
			for( int j = 0; j < G4_VIT; j++ ) vsr[ j ] = VS[ min( key0 + lane + 64 * j, lastRow ) ];

#pragma unroll
			for( int qq = 0; qq < NQ2; qq++ )
			{
				float m = mxl[ qq ];
#pragma unroll
				for( int o = 16; o > 0; o >>= 1 ) m = fmaxf( m, __shfl_xor( m, o, 64 ) );
				if( j32 == 0 && 2 * qq + g < NQ ) L.shf[ 2 * qq + g ][ wave ] = m;
			}
			__syncthreads();	// also publishes sc
			float mx[ NQ ];
#pragma unroll
			for( int q = 0; q < NQ; q++ )
			{
				float m = L.shf[ q ][ 0 ];
#pragma unroll
				for( int w = 1; w < NW; w++ ) m = fmaxf( m, L.shf[ q ][ w ] );
				mx[ q ] = m;
			}

			// ---- table softmax (ggml.c:5030-5090) over the wave's own keys: e = exp16( s - max ), double sum; p = e * scaleV[ key ] leaves as three int8 terms ----
			int psum[ NQ ];		 // sum over the wave's keys of rint( 65536 p / sp )
			float psc[ NQ ];	 // sp
#pragma unroll
			for( int q = 0; q < NQ; q++ )
			{
				double sum = 0.0;
				float p[ G4_VIT ];
				float pmax = 0.0f;
#pragma unroll
				for( int j = 0; j < G4_VIT; j++ )
				{
					const int key = key0 + lane + 64 * j;
					p[ j ] = 0.0f;
					if( key < nk )
					{
						const float e = exp16( L.sc[ q ][ key ] - mx[ q ] );
						sum += (double)e;
						p[ j ] = e * vsr[ j ];
					}
					pmax = fmaxf( pmax, p[ j ] );
				}
				float inv16;
				termScale( waveReduceMax( pmax ), psc[ q ], inv16 );
				int tot = 0;
#pragma unroll
				for( int j = 0; j < G4_VIT; j++ )
				{
					const int X = (int)rintf( p[ j ] * inv16 );
					int t[ 3 ];
					splitTerms( X, t[ 0 ], t[ 1 ], t[ 2 ] );
#pragma unroll
					for( int e = 0; e < 3; e++ ) L.pt[ wave ][ q ][ e ][ lane + 64 * j ] = (int8_t)t[ e ];
					tot += X;
				}
				psum[ q ] = waveReduceSumI( tot );
				sum = waveReduceSumD( sum );
				if( lane == 0 ) L.shd[ q ][ wave ] = sum;
			}
			__syncthreads();

			// ---- P.V: rows = terms of p (row j32 = 4 q + term), columns = dims j32 (+ 32 dh), k = the keys of a 64-key block: 32 g + 16 z + byte ----
			i32x16 o0 = {}, o1 = {};
#pragma unroll
			for( int kb = 0; kb < G4_VIT; kb++ )
			{
				if( key0 + kb * 64 >= nk ) continue;	// wave-uniform
				i32x4 pa0 = { 0, 0, 0, 0 }, pa1 = { 0, 0, 0, 0 };
				if( rowUsed )
				{
					pa0 = *(const i32x4*)( &L.pt[ wave ][ rq ][ term ][ kb * 64 + 32 * g ] );
					pa1 = *(const i32x4*)( &L.pt[ wave ][ rq ][ term ][ kb * 64 + 32 * g + 16 ] );
				}
				o0 = __builtin_amdgcn_mfma_i32_32x32x32_i8( pa0, unpackNibbles( vr[ kb ][ 0 ][ 0 ], vr[ kb ][ 0 ][ 1 ] ), o0, 0, 0, 0 );
				o0 = __builtin_amdgcn_mfma_i32_32x32x32_i8( pa1, unpackNibbles( vr[ kb ][ 0 ][ 2 ], vr[ kb ][ 0 ][ 3 ] ), o0, 0, 0, 0 );
				o1 = __builtin_amdgcn_mfma_i32_32x32x32_i8( pa0, unpackNibbles( vr[ kb ][ 1 ][ 0 ], vr[ kb ][ 1 ][ 1 ] ), o1, 0, 0, 0 );
				o1 = __builtin_amdgcn_mfma_i32_32x32x32_i8( pa1, unpackNibbles( vr[ kb ][ 1 ][ 2 ], vr[ kb ][ 1 ][ 3 ] ), o1, 0, 0, 0 );
			}
			// the wave's row of query 2 qq + g: ( 65536 A + 256 B + C - 8 sum X ) sp / 65536, exact in FP64, one rounding to FP32
#pragma unroll
			for( int qq = 0; qq < NQ2; qq++ )
			{
				const int q = 2 * qq + g;
				if( q >= NQ ) continue;
				const int qs = min( 2 * qq + 1, NQ - 1 );
				const double off = 8.0 * (double)( g ? psum[ qs ] : psum[ 2 * qq ] );
				const double sp = (double)( g ? psc[ qs ] : psc[ 2 * qq ] ) * 0x1p-16;
				const double r0 = ( (double)o0[ 4 * qq ] * 65536.0 + (double)o0[ 4 * qq + 1 ] * 256.0 + (double)o0[ 4 * qq + 2 ] - off ) * sp;
				const double r1 = ( (double)o1[ 4 * qq ] * 65536.0 + (double)o1[ 4 * qq + 1 ] * 256.0 + (double)o1[ 4 * qq + 2 ] - off ) * sp;
				L.red[ q ][ wave ][ j32 ] = (float)r0;
				L.red[ q ][ wave ][ 32 + j32 ] = (float)r1;
			}
			__syncthreads();
			if( tid < HEAD_DIM * NQ )
			{
				const int q = tid / HEAD_DIM, j = tid - q * HEAD_DIM;
				double tot = L.shd[ q ][ 0 ];
				float t = L.red[ q ][ 0 ][ j ];
#pragma unroll
				for( int w = 1; w < NW; w++ )
				{
					tot += L.shd[ q ][ w ];
					t += L.red[ q ][ w ][ j ];
				}
				a.out[ rowOf( q ) * d + h * HEAD_DIM + j ] = (f16)( t * (float)( 1.0 / tot ) );
			}
		}

		template<int NQ, bool FUSEQ, bool NT_LOADS = false>
		int launchDecG4( const DecAttnArgs& a, hipStream_t stream )
		{
			constexpr int lds = (int)sizeof( DecG4Lds<NQ> );
			static_assert( lds <= 160 * 1024, "attentionDecG4 LDS" );
			return launchLds<attentionDecG4<NQ, FUSEQ, NT_LOADS>>( dim3( a.H, a.batch / NQ, a.nTok ), dim3( NT ), lds, stream, a );
		}
	}	// namespace

	int launchQuantizeCrossKV4( const f16* srcK, uint8_t* dstK, float* scaleK, const f16* srcV, uint8_t* dstV, float* scaleV, long long heads, int T, hipStream_t stream )
	{
		if( heads <= 0 || heads > 65535 || T <= 0 || ( !dstK && !dstV ) || ( dstK && ( !srcK || !scaleK ) ) || ( dstV && ( !srcV || !scaleV ) ) ||
			( ( (size_t)srcK | (size_t)srcV | (size_t)dstK | (size_t)dstV ) % 16 ) != 0 )
		{
			setError( "quantizeCrossKV4: null, misaligned or empty operand" );
			return -1;
		}
		Quant4Args q = { { srcK, srcV }, { dstK, dstV }, { scaleK, scaleV }, T };
		hipLaunchKernelGGL( quantizeCrossKV4, dim3( (unsigned)( ( T + 63 ) / 64 ), (unsigned)heads, 2 ), dim3( Q4_NT ), 0, stream, q );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	// launchAttentionDec's branch for DecAttnArgs that carry nibble caches: cross-attention only (all keys visible)
	int launchAttentionDec4( const DecAttnArgs& a, hipStream_t stream )
	{
		const int group = a.group > 0 ? a.group : 1;
		const bool fuse = a.lnX != nullptr;
		if( !a.kc4 || !a.vc4 || !a.kScale || !a.vScale || a.causal || a.parityThreads > 0 )
		{
			setError( "attentionDec: INT4 caches serve the cross-attention only (no causal mask, no parity emulation)" );
			return -1;
		}
		if( a.nKeys <= 0 || a.nKeys > MAX_KEYS || a.nKeys > a.keyStride || a.nTok <= 0 || a.batch <= 0 )
		{
			setError( "attentionDec: key count out of range" );
			return -1;
		}
		if( ( a.batch % group ) != 0 || ( fuse && ( a.H * HEAD_DIM > G4_MAXD || ( a.H * HEAD_DIM ) % 64 != 0 ) ) || ( !fuse && !a.q ) ||
			( ( (size_t)a.kc4 | (size_t)a.vc4 ) % 16 ) != 0 )
		{
			setError( "attentionDec: unsupported group / fused-query configuration" );
			return -1;
		}
		if( group == 1 && fuse && ( g_tuning & TUNE_ATTN_DEC_NT ) ) return launchDecG4<1, true, true>( a, stream );
	#define WH_DECG4( N ) case N: return fuse ? launchDecG4<N, true>( a, stream ) : launchDecG4<N, false>( a, stream );
		switch( group )
		{
			WH_DECG4( 1 )
			WH_DECG4( 2 )
			WH_DECG4( 3 )
			WH_DECG4( 4 )
			WH_DECG4( 5 )
			WH_DECG4( 8 )
		}
	#undef WH_DECG4
		setError( "attentionDec: hypothesis groups of 1, 2, 3, 4, 5 or 8 rows are supported" );
		return -1;
	}
}
