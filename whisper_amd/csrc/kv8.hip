// FP8 cross-attention caches (wh_context_create_kv8): the quantizer behind the encoder's cross-K/V product and the decode step's
// cross-attention over the byte caches.
//
// Format. Elements are OCP FP8 E4M3 (e4m3fn: maximum 448, no infinities -- what gfx950's conversion instructions produce and consume),
// [layer][window][head][T][64], one byte each: a key row of a head is 64 contiguous bytes. One FP32 scale per key row, [layer][window][head][T],
// for K and for V separately. The scale is the power of two s = 2^ceil( log2( amax / 448 ) ) of the row's largest magnitude (1 for a row of
// zeros), so x / s and byte * s are exact and the ONE rounding is the E4M3 conversion of x / s (to nearest even); amax / s <= 448, nothing saturates.
//
// The decode kernel is attentionDecG's arithmetic (attn_dec.hip) over rows of half the bytes: FOUR lanes own a 64-byte row (16 bytes each), a wave
// instruction covers 16 whole rows = 1 KiB contiguous, a workgroup 128 rows, 12 iterations for 1536 keys -- all twelve 16-byte loads of a thread are
// requested before the first is used. Inner loop on the packed path: a pair of bytes -> packed FP16 (exact: v_cvt_scalef32_pk_f16_fp8 with scale 1) ->
// v_dot2_f32_f16 against the query's FP16 pair (the query IS an FP16 value), one convert and one dot per two elements; the row scale multiplies the
// finished dot product. P.V: the V row's scale is folded into p (one multiply per key, in the softmax pass), V pairs go bytes -> FP32 (v_cvt_pk_f32_fp8,
// exact) -> fmaf. Softmax as attentionDecG: scores in LDS, maximum, exp16, double sum.
#include "kernels.h"

namespace wh
{
	namespace
	{
		constexpr int MAX_KEYS = 1536;
		constexpr int NT = 512;
		constexpr int NW = NT / 64;
		constexpr int G8_MAXD = 1280;
		constexpr int G8_ROWS = NT / 4;				// rows one load instruction of the workgroup covers (128)
		constexpr int G8_ITERS = MAX_KEYS / G8_ROWS;	// 12
		constexpr int G8_A = 8, G8_B = G8_ITERS - G8_A;	// the two register batches: iterations 0 .. 7 and 8 .. 11
		constexpr int KPT = MAX_KEYS / NT;				// keys a thread owns in the softmax pass (tid, tid + 512, tid + 1024)

		// ---------------------------------------------------------------------------------------------------------------
		// quantizeCrossKV: FP16 rows of 64 -> E4M3 bytes + one power-of-two scale per row. 8 lanes own a 128-byte row (16-byte loads, consecutive
		// across lanes), the row's amax over them by three xor-shuffles, 8 bytes stored per lane: a wave instruction reads 8 whole rows and writes
		// 8 whole rows without gaps. A 256-thread workgroup takes QZ_U batches of 32 rows, every load requested before the first conversion.
		// blockIdx.y selects the set (K, V).
		// ---------------------------------------------------------------------------------------------------------------
		constexpr int QZ_NT = 256, QZ_U = 4, QZ_ROWS = QZ_NT / 8 * QZ_U;
		struct QuantArgs
		{
			const f16* src[ 2 ];
			uint8_t* dst[ 2 ];
			float* scale[ 2 ];
			long long rows;
		};

		__device__ __forceinline__ float xorMax8( float v )
		{
			v = fmaxf( v, __shfl_xor( v, 1, 64 ) );
			v = fmaxf( v, __shfl_xor( v, 2, 64 ) );
			v = fmaxf( v, __shfl_xor( v, 4, 64 ) );
			return v;
		}

		// 1 / s for s = the smallest power of two with 448 s >= amax (amax > 0, a finite FP16 value): 448 = 1.75 * 2^8, so with amax = m * 2^x, 1 <= m < 2,
		// s = 2^( x - 8 ) when m <= 1.75 and 2^( x - 7 ) beyond. Both s and 1 / s are normal FP32 numbers for every FP16 amax (2^-32 .. 2^8).
		__device__ __forceinline__ void rowScale( float amax, float& s, float& inv )
		{
			if( amax == 0.0f ) { s = inv = 1.0f; return; }
			const unsigned bits = __builtin_bit_cast( unsigned, amax );
			const int e = (int)( bits >> 23 ) - 127 - 8 + ( ( bits & 0x7fffffu ) > 0x600000u ? 1 : 0 );
			s = __builtin_bit_cast( float, (unsigned)( e + 127 ) << 23 );
			inv = __builtin_bit_cast( float, (unsigned)( 127 - e ) << 23 );
		}

		__global__ void __launch_bounds__( QZ_NT ) quantizeCrossKV( const QuantArgs a )
		{
			const int tid = threadIdx.x, c = tid & 7;
			const int set = blockIdx.y;
			const f16* const src = a.src[ set ];
			const long long row0 = (long long)blockIdx.x * QZ_ROWS + ( tid >> 3 );
			f16x8 x[ QZ_U ];
	#pragma unroll
			for( int u = 0; u < QZ_U; u++ )
			{
				long long row = row0 + u * ( QZ_NT / 8 );
				row = row < a.rows ? row : a.rows - 1;
				x[ u ] = __builtin_nontemporal_load( (const f16x8*)( src + row * HEAD_DIM + c * 8 ) );
			}
	#pragma unroll
			for( int u = 0; u < QZ_U; u++ )
			{
				const long long row = row0 + u * ( QZ_NT / 8 );
				float f[ 8 ];
				float amax = 0.0f;
	#pragma unroll
				for( int e = 0; e < 8; e++ )
				{
					f[ e ] = (float)x[ u ][ e ];
					amax = fmaxf( amax, fabsf( f[ e ] ) );
				}
				amax = xorMax8( amax );
				float s, inv;
				rowScale( amax, s, inv );
				u32x2 out;
	#pragma unroll
				for( int w = 0; w < 2; w++ )
				{
					int p = __builtin_amdgcn_cvt_pk_fp8_f32( f[ 4 * w ] * inv, f[ 4 * w + 1 ] * inv, 0, false );
					p = __builtin_amdgcn_cvt_pk_fp8_f32( f[ 4 * w + 2 ] * inv, f[ 4 * w + 3 ] * inv, p, true );
					out[ w ] = (unsigned)p;
				}
				if( row < a.rows )
				{
					*(u32x2*)( a.dst[ set ] + row * HEAD_DIM + c * 8 ) = out;
					if( c == 0 ) a.scale[ set ][ row ] = s;
				}
			}
		}

		// ---------------------------------------------------------------------------------------------------------------
		// attentionDecG8
		// ---------------------------------------------------------------------------------------------------------------
		template<int NQ>
		struct DecG8Lds
		{
			float sc[ NQ ][ MAX_KEYS ];
			float ks[ MAX_KEYS ];	  // the K rows' scales
			float qs[ NQ ][ HEAD_DIM ];
			float red[ NQ ][ NW ][ HEAD_DIM ];
			float shf[ NQ ][ NW ];
			double shd[ NQ ][ NW ];
			f16 xn[ NQ ][ G8_MAXD ];
		};

		__device__ __forceinline__ float xorReduce8( float v )
		{
			v += __shfl_xor( v, 1, 64 );
			v += __shfl_xor( v, 2, 64 );
			v += __shfl_xor( v, 4, 64 );
			return v;
		}

		// NT_LOADS as in attentionDecG: every row is read once per launch by one workgroup
		template<bool NT_LOADS>
		__device__ __forceinline__ u32x4 loadRow16( const uint8_t* p )
		{
			if constexpr( NT_LOADS ) return __builtin_nontemporal_load( (const u32x4*)p );
			else return *(const u32x4*)p;
		}

		// Grid (head, window group, token); 512 threads. The query part (LayerNorm, projection, rounding points) is attentionDecG's, statement for statement.
		// One query row per window (every decode step of a batch): at most 128 registers, so that two workgroups share a CU.
		template<int NQ, bool FUSEQ, bool NT_LOADS = false>
		__global__ void __launch_bounds__( NT, NQ == 1 ? 4 : 2 ) attentionDecG8( const DecAttnArgs a )
		{
			extern __shared__ __attribute__( ( aligned( 16 ) ) ) unsigned char smemG8[];
			DecG8Lds<NQ>& L = *(DecG8Lds<NQ>*)smemG8;

			const int tid = threadIdx.x;
			const int lane = tid & 63;
			const int wave = tid >> 6;
			const int g = tid >> 2, c = tid & 3;	  // row slot of an iteration, 16-byte quarter of the row
			const int h = blockIdx.x, bw = blockIdx.y, i = blockIdx.z;
			const int d = a.H * HEAD_DIM;
			const long long head = ( (long long)bw * a.H + h ) * a.keyStride;
			const uint8_t* const K = a.kc8 + head * HEAD_DIM + c * 16;
			const uint8_t* const V = a.vc8 + head * HEAD_DIM + c * 16;
			const float* const KS = a.kScale + head;
			const float* const VS = a.vScale + head;
			const int nk = a.nKeys;
			const int lastRow = nk - 1;
			auto rowOf = [ & ]( int q ) -> long long { return ( (long long)bw * NQ + q ) * a.nTok + i; };

			// ---- every K row of this thread goes out before anything else (rows beyond nk are clamped), then the K scales of the keys it owns ----
			const int nIt = ( nk + G8_ROWS - 1 ) / G8_ROWS;
			u32x4 kA[ G8_A ], kB[ G8_B ];
	#pragma unroll
			for( int u = 0; u < G8_A; u++ )
			{
				const int key = min( u * G8_ROWS + g, lastRow );
				kA[ u ] = loadRow16<NT_LOADS>( K + (long long)key * HEAD_DIM );
			}
			if( nIt > G8_A )
	#pragma unroll
				for( int u = 0; u < G8_B; u++ )
				{
					const int key = min( ( G8_A + u ) * G8_ROWS + g, lastRow );
					kB[ u ] = loadRow16<NT_LOADS>( K + (long long)key * HEAD_DIM );
				}
			float ksr[ KPT ];
	#pragma unroll
			for( int j = 0; j < KPT; j++ ) ksr[ j ] = KS[ min( tid + j * NT, lastRow ) ];

			// ---- query ----
			if constexpr( FUSEQ )
			{
				// LayerNorm of the NQ residual rows, FP32 two-pass like layerNormRows (ggml.c:4098-4156 sums in double)
				const int nv = d >> 2;	  // float4 per row
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
				// q[j] = fp16( ( W[h*64 + j] . xn + bias ) * scale ): 8 lanes per weight row, 128 contiguous bytes per row and step
				const int gw = tid >> 3, cw = tid & 7;
				const f16* const wr = a.qW + ( (long long)h * HEAD_DIM + gw ) * d + cw * 8;
				float acc[ NQ ];
	#pragma unroll
				for( int q = 0; q < NQ; q++ ) acc[ q ] = 0.0f;
				const int steps = d >> 6;
				// (four weight loads at a time where attentionDecG takes eight: the twelve K loads hold 48 registers here; the sums and their order are the same)
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
	#pragma unroll
			for( int j = 0; j < KPT; j++ ) L.ks[ tid + j * NT ] = ksr[ j ];
			__syncthreads();
			// the query's 16 dims of this lane as 8 FP16 pairs (exact: qs holds FP16 values)
			f16x2 qh[ NQ ][ 8 ];
	#pragma unroll
			for( int q = 0; q < NQ; q++ )
	#pragma unroll
				for( int e = 0; e < 8; e++ ) qh[ q ][ e ] = f16x2{ (f16)L.qs[ q ][ c * 16 + 2 * e ], (f16)L.qs[ q ][ c * 16 + 2 * e + 1 ] };

			// ---- scores ----
			float mx[ NQ ];
	#pragma unroll
			for( int q = 0; q < NQ; q++ ) mx[ q ] = -INFINITY;
			auto scoreRow = [ & ]( const u32x4& kv, int it )
			{
				const int key = it * G8_ROWS + g;
				const float ks = L.ks[ key ];
				f16x2 kp[ 8 ];
	#pragma unroll
				for( int w = 0; w < 4; w++ )
				{
					kp[ 2 * w ] = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8( (int)kv[ w ], 1.0f, false );
					kp[ 2 * w + 1 ] = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8( (int)kv[ w ], 1.0f, true );
				}
	#pragma unroll
				for( int q = 0; q < NQ; q++ )
				{
					float sacc = 0.0f;
	#pragma unroll
					for( int e = 0; e < 8; e++ ) sacc = __builtin_amdgcn_fdot2( kp[ e ], qh[ q ][ e ], sacc, false );
					sacc += __shfl_xor( sacc, 1, 64 );
					sacc += __shfl_xor( sacc, 2, 64 );
					sacc *= ks;
					if( key < nk )
					{
						mx[ q ] = fmaxf( mx[ q ], sacc );
						if( c == ( q & 3 ) ) L.sc[ q ][ key ] = sacc;
					}
				}
			};
	#pragma unroll
			for( int u = 0; u < G8_A; u++ )
				if( u < nIt ) scoreRow( kA[ u ], u );

			// the V rows of the first batch go out now: they do not depend on the softmax; so do the V scales of the keys this thread owns
			u32x4 vA[ G8_A ], vB[ G8_B ];
	#pragma unroll
			for( int u = 0; u < G8_A; u++ )
			{
				const int key = min( u * G8_ROWS + g, lastRow );
				vA[ u ] = loadRow16<NT_LOADS>( V + (long long)key * HEAD_DIM );
			}
			float vsr[ KPT ];
	#pragma unroll
			for( int j = 0; j < KPT; j++ ) vsr[ j ] = VS[ min( tid + j * NT, lastRow ) ];

			if( nIt > G8_A )
	#pragma unroll
				for( int u = 0; u < G8_B; u++ )
					if( G8_A + u < nIt ) scoreRow( kB[ u ], G8_A + u );
			if( nIt > G8_A )
	#pragma unroll
				for( int u = 0; u < G8_B; u++ )
				{
					const int key = min( ( G8_A + u ) * G8_ROWS + g, lastRow );
					vB[ u ] = loadRow16<NT_LOADS>( V + (long long)key * HEAD_DIM );
				}

	#pragma unroll
			for( int q = 0; q < NQ; q++ ) mx[ q ] = waveReduceMax( mx[ q ] );
			if( lane == 0 )
	#pragma unroll
				for( int q = 0; q < NQ; q++ ) L.shf[ q ][ wave ] = mx[ q ];
			__syncthreads();	// also publishes sc
	#pragma unroll
			for( int q = 0; q < NQ; q++ )
			{
				float m = L.shf[ q ][ 0 ];
	#pragma unroll
				for( int w = 1; w < NW; w++ ) m = fmaxf( m, L.shf[ q ][ w ] );
				mx[ q ] = m;
			}

			// ---- table softmax (ggml.c:5030-5090): e = exp16( s - max ), double sum; what is left in LDS is e * scaleV[ key ] (a power of two: exact) ----
			double sum[ NQ ];
	#pragma unroll
			for( int q = 0; q < NQ; q++ )
			{
				sum[ q ] = 0.0;
	#pragma unroll
				for( int j = 0; j < KPT; j++ )
				{
					const int key = tid + j * NT;
					if( key < nk )
					{
						const float e = exp16( L.sc[ q ][ key ] - mx[ q ] );
						L.sc[ q ][ key ] = e * vsr[ j ];
						sum[ q ] += (double)e;
					}
				}
				sum[ q ] = waveReduceSumD( sum[ q ] );
			}
			if( lane == 0 )
	#pragma unroll
				for( int q = 0; q < NQ; q++ ) L.shd[ q ][ wave ] = sum[ q ];
			__syncthreads();
			float inv[ NQ ];
	#pragma unroll
			for( int q = 0; q < NQ; q++ )
			{
				double tot = L.shd[ q ][ 0 ];
	#pragma unroll
				for( int w = 1; w < NW; w++ ) tot += L.shd[ q ][ w ];
				inv[ q ] = (float)( 1.0 / tot );
			}

			// ---- P.V, FP32: slot g owns keys g, g + 128, ...; lane c owns dims c*16 .. c*16+15 ----
			float acc[ NQ ][ 16 ];
	#pragma unroll
			for( int q = 0; q < NQ; q++ )
	#pragma unroll
				for( int e = 0; e < 16; e++ ) acc[ q ][ e ] = 0.0f;
			auto pvRow = [ & ]( const u32x4& vv, int it )
			{
				const int key = it * G8_ROWS + g;
				float vf[ 16 ];
	#pragma unroll
				for( int w = 0; w < 4; w++ )
				{
					const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8( (int)vv[ w ], false );
					const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8( (int)vv[ w ], true );
					vf[ 4 * w ] = lo[ 0 ]; vf[ 4 * w + 1 ] = lo[ 1 ]; vf[ 4 * w + 2 ] = hi[ 0 ]; vf[ 4 * w + 3 ] = hi[ 1 ];
				}
	#pragma unroll
				for( int q = 0; q < NQ; q++ )
				{
					const float p = key < nk ? L.sc[ q ][ key ] * inv[ q ] : 0.0f;
	#pragma unroll
					for( int e = 0; e < 16; e++ ) acc[ q ][ e ] = fmaf( vf[ e ], p, acc[ q ][ e ] );
				}
			};
	#pragma unroll
			for( int u = 0; u < G8_A; u++ )
				if( u < nIt ) pvRow( vA[ u ], u );
			if( nIt > G8_A )
	#pragma unroll
				for( int u = 0; u < G8_B; u++ )
					if( G8_A + u < nIt ) pvRow( vB[ u ], G8_A + u );
			// the 16 slots of a wave first (lanes with equal c), then the 8 waves through LDS in a fixed order
	#pragma unroll
			for( int q = 0; q < NQ; q++ )
	#pragma unroll
				for( int e = 0; e < 16; e++ )
				{
					float t = acc[ q ][ e ];
					t += __shfl_xor( t, 4, 64 );
					t += __shfl_xor( t, 8, 64 );
					t += __shfl_xor( t, 16, 64 );
					t += __shfl_xor( t, 32, 64 );
					acc[ q ][ e ] = t;
				}
			if( lane < 4 )
	#pragma unroll
				for( int q = 0; q < NQ; q++ )
	#pragma unroll
					for( int e = 0; e < 16; e++ ) L.red[ q ][ wave ][ lane * 16 + e ] = acc[ q ][ e ];
			__syncthreads();
			if( tid < HEAD_DIM * NQ )
			{
				const int q = tid / HEAD_DIM, j = tid - q * HEAD_DIM;
				float t = L.red[ q ][ 0 ][ j ];
	#pragma unroll
				for( int w = 1; w < NW; w++ ) t += L.red[ q ][ w ][ j ];
				a.out[ rowOf( q ) * d + h * HEAD_DIM + j ] = (f16)t;
			}
		}

		template<int NQ, bool FUSEQ, bool NT_LOADS = false>
		int launchDecG8( const DecAttnArgs& a, hipStream_t stream )
		{
			constexpr int lds = (int)sizeof( DecG8Lds<NQ> );
			static_assert( lds <= 160 * 1024, "attentionDecG8 LDS" );
			return launchLds<attentionDecG8<NQ, FUSEQ, NT_LOADS>>( dim3( a.H, a.batch / NQ, a.nTok ), dim3( NT ), lds, stream, a );
		}
	}	// namespace

	int launchQuantizeCrossKV( const f16* srcK, uint8_t* dstK, float* scaleK, const f16* srcV, uint8_t* dstV, float* scaleV, long long rows, hipStream_t stream )
	{
		if( !srcK || !dstK || !scaleK || rows <= 0 || rows > 0x7fffffffll * QZ_ROWS || ( srcV && ( !dstV || !scaleV ) ) ||
			( ( (size_t)srcK | (size_t)srcV ) % 16 ) != 0 || ( ( (size_t)dstK | (size_t)dstV ) % 8 ) != 0 )
		{
			setError( "quantizeCrossKV: null, misaligned or empty operand" );
			return -1;
		}
		QuantArgs q = { { srcK, srcV }, { dstK, dstV }, { scaleK, scaleV }, rows };
		hipLaunchKernelGGL( quantizeCrossKV, dim3( (unsigned)( ( rows + QZ_ROWS - 1 ) / QZ_ROWS ), srcV ? 2 : 1 ), dim3( QZ_NT ), 0, stream, q );
		WH_HIP( hipGetLastError() );
		return 0;
	}

	// launchAttentionDec's branch for DecAttnArgs that carry FP8 caches: cross-attention only (all keys visible, FP32 P.V)
	int launchAttentionDec8( const DecAttnArgs& a, hipStream_t stream )
	{
		const int group = a.group > 0 ? a.group : 1;
		const bool fuse = a.lnX != nullptr;
		if( !a.kc8 || !a.vc8 || !a.kScale || !a.vScale || a.causal || a.parityThreads > 0 )
		{
			setError( "attentionDec: FP8 caches serve the cross-attention only (no causal mask, no parity emulation)" );
			return -1;
		}
		if( a.nKeys <= 0 || a.nKeys > MAX_KEYS || a.nKeys > a.keyStride || a.nTok <= 0 || a.batch <= 0 )
		{
			setError( "attentionDec: key count out of range" );
			return -1;
		}
		if( ( a.batch % group ) != 0 || ( fuse && ( a.H * HEAD_DIM > G8_MAXD || ( a.H * HEAD_DIM ) % 64 != 0 ) ) || ( !fuse && !a.q ) ||
			( ( (size_t)a.kc8 | (size_t)a.vc8 ) % 16 ) != 0 )
		{
			setError( "attentionDec: unsupported group / fused-query configuration" );
			return -1;
		}
		if( group == 1 && fuse && ( g_tuning & TUNE_ATTN_DEC_NT ) ) return launchDecG8<1, true, true>( a, stream );
	#define WH_DECG8( N ) case N: return fuse ? launchDecG8<N, true>( a, stream ) : launchDecG8<N, false>( a, stream );
		switch( group )
		{
			WH_DECG8( 1 )
			WH_DECG8( 2 )
			WH_DECG8( 3 )
			WH_DECG8( 4 )
			WH_DECG8( 5 )
			WH_DECG8( 8 )
		}
	#undef WH_DECG8
		setError( "attentionDec: hypothesis groups of 1, 2, 3, 4, 5 or 8 rows are supported" );
		return -1;
	}
}
