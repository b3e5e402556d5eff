// The decode-step products (FP16 x FP16 -> FP32 on MFMA, fused epilogues): few activation rows against a weight matrix that is streamed once.
//
// gemmSkinny: M <= 32 rows when K is not a multiple of 128. The weight matrix is the MFMA A operand (32 rows per
//   workgroup), the few activation rows are the B operand; 4 waves split K and reduce through LDS.
// gemvFused: the decode-step kernel, up to 32 activation rows a row group (see below), with an optional LayerNorm prologue.
// gemmAllRows, gemmDecRows, gemmDecTile (+ decSplitCombine): the same sums for 33 .. 512 rows of a lock-step batch, each described at the kernel.
// launchGemv at the end is where a shape and the decode options (dec_lds, dec_split, vocab_lds, dec_wide_rows, dec_deep_rows, dec_tile) choose among them.
#include "gemm_device.h"
#include "gemm_launch.h"
#include <type_traits>

namespace wh
{
	namespace
	{

		// ---- skinny: M <= 32 ----
		constexpr int SK_WAVES = 4;

		template<int EPI>
		__global__ void __launch_bounds__( 256 ) gemmSkinny( const GemmArgs a )
		{
			__shared__ float red[ SK_WAVES - 1 ][ 16 ][ 64 ];

			const int tid = threadIdx.x;
			const int lane = tid & 63;
			const int wave = tid >> 6;
			const int n0 = blockIdx.x * 32;

			int n = n0 + ( lane & 31 );
			n = n < a.N ? n : a.N - 1;
			int m = lane & 31;
			m = m < a.M ? m : a.M - 1;
			const int kPer = a.K / SK_WAVES;
			const int kBeg = wave * kPer + ( lane >> 5 ) * 8;
			const f16* pw = a.W + (long long)n * a.K + kBeg;
			const f16* px = a.A + rowOffset( m, a.Mb, a.lda, a.aBatchStride ) + kBeg;

			f32x16 acc;
#pragma unroll
			for( int r = 0; r < 16; r++ ) acc[ r ] = 0.0f;

			const int steps = kPer / 16;
			int s = 0;
			for( ; s + 4 <= steps; s += 4 )
			{
				f16x8 fw[ 4 ], fx[ 4 ];
#pragma unroll
				for( int u = 0; u < 4; u++ )
				{
					fw[ u ] = __builtin_nontemporal_load( (const f16x8*)( pw + ( s + u ) * 16 ) );
					fx[ u ] = *(const f16x8*)( px + ( s + u ) * 16 );
				}
#pragma unroll
				for( int u = 0; u < 4; u++ )
					acc = __builtin_amdgcn_mfma_f32_32x32x16_f16( fw[ u ], fx[ u ], acc, 0, 0, 0 );
			}
			for( ; s < steps; s++ )
			{
				const f16x8 fw = *(const f16x8*)( pw + s * 16 );
				const f16x8 fx = *(const f16x8*)( px + s * 16 );
				acc = __builtin_amdgcn_mfma_f32_32x32x16_f16( fw, fx, acc, 0, 0, 0 );
			}

			if( wave > 0 )
			{
#pragma unroll
				for( int r = 0; r < 16; r++ ) red[ wave - 1 ][ r ][ lane ] = acc[ r ];
			}
			__syncthreads();
			if( wave != 0 ) return;
#pragma unroll
			for( int w = 0; w < SK_WAVES - 1; w++ )
#pragma unroll
				for( int r = 0; r < 16; r++ ) acc[ r ] += red[ w ][ r ][ lane ];

			// D[row][col]: row = weight row (n), col = activation row (m)
			const int mm = lane & 31;
			if( mm >= a.M ) return;
			const int hi = lane >> 5;
#pragma unroll
			for( int r = 0; r < 16; r++ )
			{
				const int nn = n0 + ( r & 3 ) + 8 * ( r >> 2 ) + 4 * hi;
				if( nn < a.N )
					epilogueOne<EPI>( a, mm, nn, acc[ r ] );
			}
		}
		// ---- gemv: M <= 32 activation rows (single-token decode steps of a lock-step batch; MT = 2 above 16 rows) ----
		// HBM/latency-bound: the only thing that matters is how many weight bytes are in flight. 16 weight rows per
		// workgroup (N/16 workgroups), 4 waves split K, and every wave issues ALL of its weight loads (16 bytes per lane
		// each, up to GV_UNROLL (8 or 16) at a time) before the first MFMA consumes one. v_mfma_f32_16x16x32_f16: A = 16 weight rows,
		// B = up to 16 activation rows. With lnX != null the LayerNorm that precedes the product in the graph
		// (norm.hlsl + fmaRepeat1.hlsl in the reference) runs as a prologue: each workgroup normalises the M rows into LDS
		// (FP16, the rounding the product applies anyway) -- M*K*4 bytes of L2 reads per workgroup instead of a launch.
		constexpr int GV_UNROLL_MAX = 16;
		constexpr int GV_MAXK_LN = 1280;
		constexpr int GV_XS_STRIDE = GV_MAXK_LN + 8;

		// LayerNorm + affine of up to RB rows by the WHOLE workgroup (NWV waves): thread t owns the float4 columns t and
		// t + 64 * NWV of every row, so a row is one coalesced pass and all RB rows are in flight at once; the two reductions go
		// wave-shuffle -> LDS -> every thread. Same formula as layerNormRows (two-pass FP32, eps 1e-5, w*y + b, FP16 result);
		// the summation tree differs, so rows are not bit-identical with the one-wave-per-row version.
		template<int RB, int MAXC, int NWV, class Store>
		__device__ __forceinline__ void layerNormBlock( const float* __restrict__ x, int nRows, const float* __restrict__ w, const float* __restrict__ b,
			int d, int tid, float ( *shA )[ RB ], float ( *shB )[ RB ], Store&& store )
		{
			constexpr int NTH = NWV * 64;
			const int lane = tid & 63, wave = tid >> 6;
			const int nv = d >> 2;
			f32x4 v[ RB ][ MAXC ], wv[ MAXC ], bv[ MAXC ];
	#pragma unroll
			for( int i = 0; i < MAXC; i++ )
			{
				const int cv = tid + i * NTH;
				const int cc = ( cv < nv ? cv : nv - 1 ) * 4;
				wv[ i ] = *(const f32x4*)( w + cc );
				bv[ i ] = *(const f32x4*)( b + cc );
	#pragma unroll
				for( int r = 0; r < RB; r++ )
				{
					const int rr = r < nRows ? r : ( nRows > 0 ? nRows - 1 : 0 );
					v[ r ][ i ] = *(const f32x4*)( x + (long long)rr * d + cc );
				}
			}
			const float invD = 1.0f / (float)d;
			float s[ RB ];
	#pragma unroll
			for( int r = 0; r < RB; r++ )
			{
				float t = 0.0f;
	#pragma unroll
				for( int i = 0; i < MAXC; i++ )
					if( tid + i * NTH < nv ) t += ( v[ r ][ i ][ 0 ] + v[ r ][ i ][ 1 ] ) + ( v[ r ][ i ][ 2 ] + v[ r ][ i ][ 3 ] );
				s[ r ] = t;
			}
	#pragma unroll
			for( int o = 32; o > 0; o >>= 1 )
	#pragma unroll
				for( int r = 0; r < RB; r++ ) s[ r ] += __shfl_xor( s[ r ], o, 64 );
			if( lane == 0 )
	#pragma unroll
				for( int r = 0; r < RB; r++ ) shA[ wave ][ r ] = s[ r ];
			__syncthreads();
	#pragma unroll
			for( int r = 0; r < RB; r++ )
			{
				float t = shA[ 0 ][ r ];
	#pragma unroll
				for( int ww = 1; ww < NWV; ww++ ) t += shA[ ww ][ r ];
				const float mean = t * invD;
				float q = 0.0f;
	#pragma unroll
				for( int i = 0; i < MAXC; i++ )
				{
	#pragma unroll
					for( int e = 0; e < 4; e++ ) v[ r ][ i ][ e ] -= mean;
					if( tid + i * NTH < nv )
	#pragma unroll
						for( int e = 0; e < 4; e++ ) q = fmaf( v[ r ][ i ][ e ], v[ r ][ i ][ e ], q );
				}
				s[ r ] = q;
			}
	#pragma unroll
			for( int o = 32; o > 0; o >>= 1 )
	#pragma unroll
				for( int r = 0; r < RB; r++ ) s[ r ] += __shfl_xor( s[ r ], o, 64 );
			if( lane == 0 )
	#pragma unroll
				for( int r = 0; r < RB; r++ ) shB[ wave ][ r ] = s[ r ];
			__syncthreads();
	#pragma unroll
			for( int r = 0; r < RB; r++ )
			{
				if( r >= nRows ) continue;
				float t = shB[ 0 ][ r ];
	#pragma unroll
				for( int ww = 1; ww < NWV; ww++ ) t += shB[ ww ][ r ];
				const float rstd = 1.0f / sqrtf( t * invD + 1e-5f );
	#pragma unroll
				for( int i = 0; i < MAXC; i++ )
				{
					const int cv = tid + i * NTH;
					if( cv < nv )
					{
						f16x4 hv;
	#pragma unroll
						for( int e = 0; e < 4; e++ ) hv[ e ] = (f16)__fadd_rn( __fmul_rn( __fmul_rn( v[ r ][ i ][ e ], rstd ), wv[ i ][ e ] ), bv[ i ][ e ] );
						store( r, cv * 4, hv );
					}
				}
			}
		}

		// PRO = 0: A rows are FP16 in global memory; 1: fused LayerNorm prologue, a wave per pair of rows (up to 16 rows);
		// 2: fused LayerNorm prologue by the whole workgroup, 16 rows at a time (17 .. 32 rows).
		// ROWS = weight rows per workgroup: 16 fills the MFMA; 4 (rows replicated across the operand's 16 row slots) gives 4x
		// the workgroups when N is small and K large -- a CU streams only ~24 GB/s, so 8 MB over 64 CUs would take 5 us.
		// NW = waves per workgroup that split K. GV_UNROLL = fragment slots per wave (8 halves the registers when K / NW / 32 <= 8).
		// MT = MFMA column tiles = 16 activation rows each.
		template<int EPI, int PRO, int ROWS, int NW, int GV_UNROLL, int MT>
		__global__ void __launch_bounds__( NW * 64 ) gemvFused( const GemmArgs a )
		{
			constexpr bool LN = PRO == 1;
			__shared__ float red[ NW - 1 ][ MT * 4 ][ 64 ];
			__shared__ float lnA[ PRO == 2 ? NW : 1 ][ 16 ], lnB2[ PRO == 2 ? NW : 1 ][ 16 ];
			extern __shared__ __attribute__( ( aligned( 16 ) ) ) f16 xs[];	 // [16 * MT][GV_XS_STRIDE] when there is a prologue

			const int tid = threadIdx.x;
			const int lane = tid & 63;
			const int wave = tid >> 6;
			const int n0 = blockIdx.x * ROWS;
			// more than 16 * MT activation rows: blockIdx.y selects the group of 16 * MT rows (the weight rows are streamed once
			// per group; these launches are latency-bound, the second copy comes from L2 or overlaps the first)
			const int m0 = blockIdx.y * 16 * MT;
			const int mEnd = a.M;

			int n = n0 + ( lane & 15 ) % ROWS;
			n = n < a.N ? n : a.N - 1;
			const int kPer = a.K / NW;
			const int kBeg = wave * kPer + ( lane >> 4 ) * 8;
			const f16* const pw = a.W + (long long)n * a.K + kBeg;
			const int steps = kPer / 32;

			// first batch of weight loads goes out before anything else: it does not depend on the LayerNorm prologue
			f16x8 fw[ GV_UNROLL ], fx[ MT ][ GV_UNROLL ];
#pragma unroll
			for( int u = 0; u < GV_UNROLL; u++ )
				if( u < steps ) fw[ u ] = __builtin_nontemporal_load( (const f16x8*)( pw + u * 32 ) );

			// epilogue operands of the plain FP32 epilogue are fetched up front as well (wave 0 owns the epilogue)
			const int nEp = n0 + ( lane >> 4 ) * 4;
			const bool fastEp = EPI == EPI_F32 && ( a.N & 15 ) == 0 && a.Mb >= a.M;
			const bool ownsRows = ( lane >> 4 ) * 4 < ROWS;	  // with ROWS == 4 only the first 16 lanes hold distinct output rows
			f32x4 biasv = { 0.0f, 0.0f, 0.0f, 0.0f }, resv[ MT ];
#pragma unroll
			for( int t = 0; t < MT; t++ ) resv[ t ] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
			if( fastEp && wave == 0 && ownsRows )
			{
				if( a.bias ) biasv = *(const f32x4*)( a.bias + nEp );
#pragma unroll
				for( int t = 0; t < MT; t++ )
					if( a.res && m0 + t * 16 + ( lane & 15 ) < mEnd ) resv[ t ] = *(const f32x4*)( a.res + (long long)( m0 + t * 16 + ( lane & 15 ) ) * a.ldc + nEp );
			}

			const f16* px[ MT ];
			if constexpr( LN )
			{
				// rows wave and wave + NW together, then the next pair. Rows at or beyond M stay unwritten: an MFMA output
				// column depends on its own activation row only, and those columns are never stored.
				for( int r0 = wave; r0 < a.M; r0 += 2 * NW )
				{
					const int nr = ( a.M - r0 + NW - 1 ) / NW;
					layerNormRows<GV_MAXK_LN / 256, 2>( a.lnX + (long long)r0 * a.K, (long long)NW * a.K, nr, a.lnW, a.lnB, a.K, lane,
						[ = ]( int j, int c, f16x4 v ) { *(f16x4*)( xs + ( r0 + j * NW ) * GV_XS_STRIDE + c ) = v; } );
				}
				__syncthreads();
			}
			if constexpr( PRO == 2 )
			{
				for( int r0 = 0; r0 < a.M; r0 += 16 )
					layerNormBlock<16, ( GV_MAXK_LN / 4 + NW * 64 - 1 ) / ( NW * 64 ), NW>( a.lnX + (long long)r0 * a.K, a.M - r0, a.lnW, a.lnB, a.K, tid, lnA, lnB2,
						[ = ]( int j, int c, f16x4 v ) { *(f16x4*)( xs + ( r0 + j ) * GV_XS_STRIDE + c ) = v; } );
				__syncthreads();
			}
#pragma unroll
			for( int t = 0; t < MT; t++ )
			{
				if constexpr( PRO != 0 )
					px[ t ] = xs + ( t * 16 + ( lane & 15 ) ) * GV_XS_STRIDE + kBeg;
				else
				{
					int m = m0 + t * 16 + ( lane & 15 );
					m = m < mEnd ? m : mEnd - 1;
					px[ t ] = a.A + rowOffset( m, a.Mb, a.lda, a.aBatchStride ) + kBeg;
				}
			}

			f32x4 acc[ MT ];
#pragma unroll
			for( int t = 0; t < MT; t++ ) acc[ t ] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
			for( int u = 0; u < GV_UNROLL; u++ )
				if( u < steps )
				{
#pragma unroll
					for( int t = 0; t < MT; t++ ) fx[ t ][ u ] = *(const f16x8*)( px[ t ] + u * 32 );
				}
#pragma unroll
			for( int u = 0; u < GV_UNROLL; u++ )
				if( u < steps )
				{
#pragma unroll
					for( int t = 0; t < MT; t++ ) acc[ t ] = __builtin_amdgcn_mfma_f32_16x16x32_f16( fw[ u ], fx[ t ][ u ], acc[ t ], 0, 0, 0 );
				}
			for( int s = GV_UNROLL; s < steps; s += GV_UNROLL )
			{
#pragma unroll
				for( int u = 0; u < GV_UNROLL; u++ )
					if( s + u < steps )
					{
						fw[ u ] = __builtin_nontemporal_load( (const f16x8*)( pw + ( s + u ) * 32 ) );
#pragma unroll
						for( int t = 0; t < MT; t++ ) fx[ t ][ u ] = *(const f16x8*)( px[ t ] + ( s + u ) * 32 );
					}
#pragma unroll
				for( int u = 0; u < GV_UNROLL; u++ )
					if( s + u < steps )
					{
#pragma unroll
						for( int t = 0; t < MT; t++ ) acc[ t ] = __builtin_amdgcn_mfma_f32_16x16x32_f16( fw[ u ], fx[ t ][ u ], acc[ t ], 0, 0, 0 );
					}
			}

			if( wave > 0 )
			{
#pragma unroll
				for( int t = 0; t < MT; t++ )
#pragma unroll
					for( int r = 0; r < 4; r++ ) red[ wave - 1 ][ t * 4 + r ][ lane ] = acc[ t ][ r ];
			}
			__syncthreads();
			if( wave != 0 ) return;
#pragma unroll
			for( int w = 0; w < NW - 1; w++ )
#pragma unroll
				for( int t = 0; t < MT; t++ )
#pragma unroll
					for( int r = 0; r < 4; r++ ) acc[ t ][ r ] += red[ w ][ t * 4 + r ][ lane ];

			// D[row][col]: col = lane & 15 = activation row within the tile, row = (lane >> 4) * 4 + r = weight row slot
			if( !ownsRows ) return;
#pragma unroll
			for( int t = 0; t < MT; t++ )
			{
				const int mm = m0 + t * 16 + ( lane & 15 );
				if( mm >= mEnd ) continue;
				if( fastEp )
				{
					// out = (acc + bias) + res, the same order as epilogueOne<EPI_F32>
					f32x4 o;
#pragma unroll
					for( int r = 0; r < 4; r++ ) o[ r ] = ( acc[ t ][ r ] + biasv[ r ] ) + resv[ t ][ r ];
					*(f32x4*)( a.out32 + (long long)mm * a.ldc + nEp ) = o;
					continue;
				}
#pragma unroll
				for( int r = 0; r < 4; r++ )
				{
					const int nn = n0 + ( lane >> 4 ) * 4 + r;
					if( nn < a.N )
						epilogueOne<EPI>( a, mm, nn, acc[ t ][ r ] );
				}
			}
		}

		// -----------------------------------------------------------------------------------------------------------
		// gemmAllRows: 33 .. 128 activation rows against a WIDE weight matrix (the vocabulary projection of a decode step:
		// N = 51865). A workgroup owns 32 columns x ALL rows: the weights are fetched once (gemvFused fetches them once per
		// group of 64 rows) and the activation rows are re-read once per 32 columns instead of once per 16. The 4 waves split
		// K; a wave keeps MT x 2 MFMA 16x16x32 tiles and has two k-steps of loads (2 weight + MT activation fragments each)
		// in flight; the 4 partial tiles meet in LDS and wave w finishes accumulator groups w, w + 4, ... in the fixed order
		// 0, 1, 2, 3. Measured at 112 rows, N = 51865, K = 1024: 112 us (950 GB/s) vs 165 us for gemvFused.
		// It needs N / 32 >= ~500 workgroups to fill the chip. Splitting K over MORE workgroups for the narrow products
		// (N = 1024: 32 column tiles) was built and measured -- partial sums to a scratch buffer, __threadfence, one atomic
		// ticket per tile, last arrival adds the slices in slice order -- and retired: the agent-scope fences (an L2 write-back
		// per workgroup on gfx950) cost 5-30 us per launch, 40-78 us against gemvFused's 8-22 us.
		template<int EPI, int MT>
		__global__ void __launch_bounds__( 256 ) gemmAllRows( const GemmArgs a )
		{
			constexpr int NW = 4, CT = 2, G = MT * CT;
			constexpr int GPW = ( G + NW - 1 ) / NW;	   // accumulator groups (4 registers x 64 lanes) a wave owns after the LDS exchange
			extern __shared__ __attribute__( ( aligned( 16 ) ) ) float redK[];	 // [NW][G * 4][64]

			const int tid = threadIdx.x;
			const int lane = tid & 63;
			const int wave = tid >> 6;
			const int tile = blockIdx.x;
			const int n0 = tile * 16 * CT;
			const int kPer = a.K / NW;
			const int kBeg = wave * kPer + ( lane >> 4 ) * 8;
			const int steps = kPer / 32;

			const f16* pw[ CT ];
	#pragma unroll
			for( int c = 0; c < CT; c++ )
			{
				int n = n0 + c * 16 + ( lane & 15 );
				n = n < a.N ? n : a.N - 1;
				pw[ c ] = a.W + (long long)n * a.K + kBeg;
			}
			const f16* px[ MT ];
	#pragma unroll
			for( int t = 0; t < MT; t++ )
			{
				int m = t * 16 + ( lane & 15 );
				m = m < a.M ? m : a.M - 1;
				px[ t ] = a.A + rowOffset( m, a.Mb, a.lda, a.aBatchStride ) + kBeg;
			}

			f32x4 acc[ MT ][ CT ];
	#pragma unroll
			for( int t = 0; t < MT; t++ )
	#pragma unroll
				for( int c = 0; c < CT; c++ ) acc[ t ][ c ] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };

			for( int s0 = 0; s0 < steps; s0 += 2 )
			{
				f16x8 fw[ 2 ][ CT ], fx[ 2 ][ MT ];
	#pragma unroll
				for( int u = 0; u < 2; u++ )
					if( s0 + u < steps )
					{
	#pragma unroll
						for( int c = 0; c < CT; c++ ) fw[ u ][ c ] = __builtin_nontemporal_load( (const f16x8*)( pw[ c ] + ( s0 + u ) * 32 ) );
	#pragma unroll
						for( int t = 0; t < MT; t++ ) fx[ u ][ t ] = *(const f16x8*)( px[ t ] + ( s0 + u ) * 32 );
					}
	#pragma unroll
				for( int u = 0; u < 2; u++ )
					if( s0 + u < steps )
					{
	#pragma unroll
						for( int t = 0; t < MT; t++ )
	#pragma unroll
							for( int c = 0; c < CT; c++ )
								acc[ t ][ c ] = __builtin_amdgcn_mfma_f32_16x16x32_f16( fw[ u ][ c ], fx[ u ][ t ], acc[ t ][ c ], 0, 0, 0 );
					}
			}

			// ---- the 4 K-quarters of the workgroup meet in LDS ----
	#pragma unroll
			for( int t = 0; t < MT; t++ )
	#pragma unroll
				for( int c = 0; c < CT; c++ )
	#pragma unroll
					for( int r = 0; r < 4; r++ ) redK[ ( wave * G * 4 + ( t * CT + c ) * 4 + r ) * 64 + lane ] = acc[ t ][ c ][ r ];
			__syncthreads();
			f32x4 part[ GPW ];
	#pragma unroll
			for( int i = 0; i < GPW; i++ )
			{
				const int g = wave + NW * i;
				if( g >= G ) continue;
	#pragma unroll
				for( int r = 0; r < 4; r++ )
				{
					float v = redK[ ( 0 * G * 4 + g * 4 + r ) * 64 + lane ];
	#pragma unroll
					for( int w = 1; w < NW; w++ ) v += redK[ ( w * G * 4 + g * 4 + r ) * 64 + lane ];
					part[ i ][ r ] = v;
				}
			}

			// ---- epilogue: group g = (row tile t, column fragment c); D[row][col]: col = lane & 15 = activation row, row = weight row slot
			const bool fastEp = EPI == EPI_F32 && ( a.N & 3 ) == 0 && a.Mb >= a.M;
	#pragma unroll
			for( int i = 0; i < GPW; i++ )
			{
				const int g = wave + NW * i;
				if( g >= G ) continue;
				const int t = g / CT, c = g - t * CT;
				const int mm = t * 16 + ( lane & 15 );
				const int nn = n0 + c * 16 + ( lane >> 4 ) * 4;
				if( mm >= a.M || nn >= a.N ) continue;
				if( fastEp )
				{
					// out = (acc + bias) + res, the same order as epilogueOne<EPI_F32>
					f32x4 o = part[ i ];
					if( a.bias )
					{
						const f32x4 bv = *(const f32x4*)( a.bias + nn );
	#pragma unroll
						for( int r = 0; r < 4; r++ ) o[ r ] += bv[ r ];
					}
					const long long off = (long long)mm * a.ldc + nn;
					if( a.res )
					{
						const f32x4 rv = *(const f32x4*)( a.res + off );
	#pragma unroll
						for( int r = 0; r < 4; r++ ) o[ r ] += rv[ r ];
					}
					*(f32x4*)( a.out32 + off ) = o;
					continue;
				}
	#pragma unroll
				for( int r = 0; r < 4; r++ )
					if( nn + r < a.N ) epilogueOne<EPI>( a, mm, nn + r, part[ i ][ r ] );
			}
		}

		// -----------------------------------------------------------------------------------------------------------
		// The epilogue of the decode-rows kernels: group g = wave + NW i of the workgroup's MT x CT tiles of 16 x 16 is in part[ i ] -- D[row][col]: col = lane & 15 =
		// activation row of the tile, row = (lane >> 4) * 4 + r = weight row slot (four consecutive output columns of one activation row per lane)
		template<int EPI, int MT, int CT, int NW>
		__device__ __forceinline__ void decRowsEpilogue( const GemmArgs& a, const f32x4 ( &part )[ ( MT * CT + NW - 1 ) / NW ], int m0, int n0, int wave, int lane )
		{
			constexpr int G = MT * CT;
			constexpr int GPW = ( G + NW - 1 ) / NW;
			const bool fast32 = EPI == EPI_F32 && ( a.N & 3 ) == 0 && a.Mb >= a.M;
			const bool fastGelu = EPI == EPI_F16_GELU && ( a.N & 3 ) == 0 && a.Mb >= a.M;
	#pragma unroll
			for( int i = 0; i < GPW; i++ )
			{
				const int g = wave + NW * i;
				if( g >= G ) continue;
				const int t = g / CT, c = g - t * CT;
				const int mm = m0 + t * 16 + ( lane & 15 );
				const int nn = n0 + c * 16 + ( lane >> 4 ) * 4;
				if( mm >= a.M || nn >= a.N ) continue;
				if( fast32 )
				{
					// out = (acc + bias) + res, the same order as epilogueOne<EPI_F32>
					f32x4 o = part[ i ];
					if( a.bias )
					{
						const f32x4 bv = *(const f32x4*)( a.bias + nn );
	#pragma unroll
						for( int r = 0; r < 4; r++ ) o[ r ] += bv[ r ];
					}
					const long long off = (long long)mm * a.ldc + nn;
					if( a.res )
					{
						const f32x4 rv = *(const f32x4*)( a.res + off );
	#pragma unroll
						for( int r = 0; r < 4; r++ ) o[ r ] += rv[ r ];
					}
					*(f32x4*)( a.out32 + off ) = o;
					continue;
				}
				if( fastGelu )
				{
					// gelu16( acc + bias ), the arithmetic of epilogueOne<EPI_F16_GELU>, four columns as one 8-byte store
					const f32x4 bv = *(const f32x4*)( a.bias + nn );
					f16x4 hv;
	#pragma unroll
					for( int r = 0; r < 4; r++ ) hv[ r ] = gelu16( part[ i ][ r ] + bv[ r ] );
					*(f16x4*)( a.out16 + (long long)mm * a.ldc + nn ) = hv;
					continue;
				}
				if constexpr( EPI == EPI_QKV_DEC )
				{
					// the arithmetic of epilogueOne<EPI_QKV_DEC> on the lane's four consecutive columns (one head, one of Q / K / V: d and HEAD_DIM are multiples of 4),
					// leaving as ONE 8-byte store: one pair of divisions and one position load per lane instead of four, a quarter of the store instructions
					if( ( a.N & 3 ) == 0 )
					{
						const int d = a.H * HEAD_DIM;
						const int sel = nn / d;
						const int c = nn - sel * d;
						f16x4 hv;
						f16* dst;
						if( sel == 0 )
						{
							const f32x4 bv = *(const f32x4*)( a.bias + nn );
	#pragma unroll
							for( int r = 0; r < 4; r++ ) hv[ r ] = (f16)( ( part[ i ][ r ] + bv[ r ] ) * a.scale );
							dst = a.q + (long long)mm * d + c;
						}
						else
						{
							const int h = c >> 6, dd = c & 63;
							const int b = mm / a.nTok;
							const int pos = ( a.nPastDev ? a.nPastDev[ b ] : a.nPast ) + ( mm - b * a.nTok );
							const long long o = ( ( (long long)b * a.H + h ) * a.textCtx + pos ) * HEAD_DIM + dd;
							if( sel == 1 )
							{
	#pragma unroll
								for( int r = 0; r < 4; r++ ) hv[ r ] = (f16)( part[ i ][ r ] * a.scale );
								dst = a.k + o;
							}
							else
							{
								const f32x4 bv = *(const f32x4*)( a.bias + nn );
	#pragma unroll
								for( int r = 0; r < 4; r++ ) hv[ r ] = (f16)( part[ i ][ r ] + bv[ r ] );
								dst = a.v + o;
							}
						}
						*(f16x4*)dst = hv;
						continue;
					}
				}
	#pragma unroll
				for( int r = 0; r < 4; r++ )
					if( nn + r < a.N ) epilogueOne<EPI>( a, mm, nn + r, part[ i ][ r ] );
			}
		}

		// gemmDecRows: the products of a decode step whose lock-step batch is LARGER than 128 sequences (129 .. 512 rows: one
		// context of 224 .. 448 windows instead of two of 112). At that many rows a product is a small GEMM (448 x 4096 x 1024:
		// 3.8 GFLOP against 8 MB of weights), and gemvFused's 16-column workgroups would re-read the activation rows once per
		// 16 columns: 64 KB of L2 -> CU traffic per 16 x 64 outputs. Here a workgroup owns 16 CT weight rows x 16 MT activation
		// rows (64 x 64 by default: 8 fragment loads feed 16 MFMAs per k-step and wave, 2.5 x fewer bytes per output), the 4
		// waves split K exactly as gemvFused's do and their partial tiles meet in LDS in wave order 0, 1, 2, 3 -- the same
		// summation order, so a row's result does not depend on which of the two kernels (or which row tile) computed it.
		// Grid (column tiles, row tiles). Operands come straight from L2 (every wave reads its own K quarter: nothing to share
		// through LDS); two k-steps of loads are in flight per wave.
		template<int EPI, int MT, int CT, int DEPTH, int NW = 4>
		__global__ void __launch_bounds__( NW * 64 ) gemmDecRows( const GemmArgs a )
		{
			// NW = waves that split K: 4, or 8 for the MLP down-projection (K = 4 d) of 33 .. 128 rows -- gemvFused's own split there (TUNE_GEMV_K8), same order
			constexpr int G = MT * CT;
			constexpr int GPW = ( G + NW - 1 ) / NW;
			extern __shared__ __attribute__( ( aligned( 16 ) ) ) float redD[];	 // [NW][G * 4][64]

			const int tid = threadIdx.x;
			const int lane = tid & 63;
			const int wave = tid >> 6;
			const int n0 = blockIdx.x * 16 * CT;
			const int m0 = blockIdx.y * 16 * MT;
			const int kPer = a.K / NW;
			const int kBeg = wave * kPer + ( lane >> 4 ) * 8;
			const int steps = kPer / 32;

			const f16* pw[ CT ];
	#pragma unroll
			for( int c = 0; c < CT; c++ )
			{
				int n = n0 + c * 16 + ( lane & 15 );
				n = n < a.N ? n : a.N - 1;
				pw[ c ] = a.W + (long long)n * a.K + kBeg;
			}
			const f16* px[ MT ];
	#pragma unroll
			for( int t = 0; t < MT; t++ )
			{
				int m = m0 + t * 16 + ( lane & 15 );
				m = m < a.M ? m : a.M - 1;
				px[ t ] = a.A + rowOffset( m, a.Mb, a.lda, a.aBatchStride ) + kBeg;
			}

			f32x4 acc[ MT ][ CT ];
	#pragma unroll
			for( int t = 0; t < MT; t++ )
	#pragma unroll
				for( int c = 0; c < CT; c++ ) acc[ t ][ c ] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };

			// software pipeline: the fragments of k-steps s + 1 .. s + DEPTH - 1 are in flight behind the MFMAs of step s (a ring of DEPTH register sets; the
			// smaller tiles have the registers for a deeper ring, and need it: fewer MFMAs per step to hide an L2 round trip behind)
			// (DEPTH: 2 at 64 x 64 -- 152 VGPRs already --, 3 at 64 x 32 / 32 x 64, 4 at 32 x 32; option dec_depth = 2 pins the round-5a pipeline for A/B runs)
			f16x8 fw[ DEPTH ][ CT ], fx[ DEPTH ][ MT ];
	#pragma unroll
			for( int d = 0; d < DEPTH - 1; d++ )
				if( d < steps )
				{
	#pragma unroll
					for( int c = 0; c < CT; c++ ) fw[ d ][ c ] = *(const f16x8*)( pw[ c ] + d * 32 );
	#pragma unroll
					for( int t = 0; t < MT; t++ ) fx[ d ][ t ] = *(const f16x8*)( px[ t ] + d * 32 );
				}
			for( int s0 = 0; s0 < steps; s0 += DEPTH )
			{
	#pragma unroll
				for( int u = 0; u < DEPTH; u++ )
				{
					const int s = s0 + u;
					if( s >= steps ) break;
					constexpr int ahead = DEPTH - 1;
					const int nxt = ( u + ahead ) % DEPTH;	  // the set step s - 1 has just released
					if( s + ahead < steps )
					{
	#pragma unroll
						for( int c = 0; c < CT; c++ ) fw[ nxt ][ c ] = *(const f16x8*)( pw[ c ] + ( s + ahead ) * 32 );
	#pragma unroll
						for( int t = 0; t < MT; t++ ) fx[ nxt ][ t ] = *(const f16x8*)( px[ t ] + ( s + ahead ) * 32 );
					}
	#pragma unroll
					for( int t = 0; t < MT; t++ )
	#pragma unroll
						for( int c = 0; c < CT; c++ )
							acc[ t ][ c ] = __builtin_amdgcn_mfma_f32_16x16x32_f16( fw[ u ][ c ], fx[ u ][ t ], acc[ t ][ c ], 0, 0, 0 );
				}
			}

			// ---- the 4 K-quarters of the workgroup meet in LDS ----
	#pragma unroll
			for( int t = 0; t < MT; t++ )
	#pragma unroll
				for( int c = 0; c < CT; c++ )
	#pragma unroll
					for( int r = 0; r < 4; r++ ) redD[ ( wave * G * 4 + ( t * CT + c ) * 4 + r ) * 64 + lane ] = acc[ t ][ c ][ r ];
			__syncthreads();
			f32x4 part[ GPW ];
	#pragma unroll
			for( int i = 0; i < GPW; i++ )
			{
				const int g = wave + NW * i;
				if( g >= G ) continue;
	#pragma unroll
				for( int r = 0; r < 4; r++ )
				{
					float v = redD[ ( 0 * G * 4 + g * 4 + r ) * 64 + lane ];
	#pragma unroll
					for( int w = 1; w < NW; w++ ) v += redD[ ( w * G * 4 + g * 4 + r ) * 64 + lane ];
					part[ i ][ r ] = v;
				}
			}

			decRowsEpilogue<EPI, MT, CT, NW>( a, part, m0, n0, wave, lane );
		}

		// gemmDecTile (round 6): the same products (129 .. 512 rows) with the operands staged through LDS in FULL 128-byte lines. gemmDecRows' waves read their
		// fragments straight from L2, 16 rows x 64 bytes per instruction -- every 128-byte line is requested twice, by different instructions, and the kernel is bound by
		// that request stream (448 x 4096 x 1024: 21 us whatever the prefetch depth, 13 us at half the rows; profiles/r06_evidence/decode_rows_r6p.txt). Here a
		// workgroup (4 waves, 64 activation rows x 16 CT weight rows) walks K in tiles of 64 = one line per row: LDS-DMA pieces of 8 rows x 128 bytes (source chunk
		// XOR-swizzled as in the encoder's kernels), a ring of DT_NBUF tiles with counted waits and one barrier per tile, fragments by ds_read_b128. Wave w owns the
		// 16-column tile w % CT of MT / (4 / CT) row tiles -- the groups g = w + 4 i of decRowsEpilogue -- so its W fragment is the srcA operand of consecutive MFMAs.
		// THE SUMS ARE gemvFused's / gemmDecRows': those kernels give every wave a quarter of K and add the four partial tiles in wave order; here every wave walks all of
		// K, but closes an accumulator at each quarter of K and adds the four in the same order: ((P0 + P1) + P2) + P3, each Pi the same chain of k-steps of 32.
		constexpr int DT_NBUF = 4;
		// SPLIT = 8 (round 6, the MLP down-projection of 33 .. 128 rows: N = d gives only N / 32 = 32 .. 40 column tiles): blockIdx.y selects an EIGHTH of K instead of
		// a row tile -- gemvFused's eight-wave K split (TUNE_GEMV_K8) dealt to eight workgroups. The FP32 partial tile P_e goes to a.splitScratch[e][M][N]; the launch
		// that follows (decSplitCombine) adds the eight in gemvFused's order, ((P0 + P1) + ... ) + P7, then bias and residual: the same bits. Two launches, no atomics
		// (a last-arrival combine needs agent-scope fences: an L2 write-back per workgroup on gfx950, 5-30 us -- see gemmAllRows).
		template<int EPI, int CT, int KS = 1, int NBUF = DT_NBUF, int MT = 4, int SPLIT = 0>
		__global__ void __launch_bounds__( 256 ) gemmDecTile( const GemmArgs a )
		{
			// KS = K tiles of 64 per ring slot and barrier (2 for the deep products: K = 4096 is 64 tiles, and a tile is only 4 .. 8 MFMAs per wave)
			// MT = row tiles of 16 per workgroup: 4, or 6 / 8 with CT = 2 for the wide products of 65 .. 128 rows (all rows in one workgroup per 32 columns)
			static_assert( CT == 4 || CT == 2, "wave w owns column tile w % CT" );
			static_assert( MT == 4 || ( CT == 2 && ( MT == 6 || MT == 8 ) ), "an even number of row tiles per column pair" );
			constexpr int NW = 4, GPW = MT * CT / NW, AP = MT / 2;	  // AP = A pieces (8 rows x 128 bytes) per wave
			constexpr int A_BYTES = MT * 16 * 128, W_BYTES = CT * 16 * 128, TILE = A_BYTES + W_BYTES, STAGE = KS * TILE;
			constexpr int P = KS * ( AP + ( CT == 4 ? 2 : 1 ) );	  // load instructions per slot and wave
			extern __shared__ __attribute__( ( aligned( 16 ) ) ) unsigned char smemD[];
			typedef __attribute__( ( address_space( 3 ) ) ) void* LdsPtr;
			const int tid = threadIdx.x;
			const int lane = tid & 63;
			const int wave = __builtin_amdgcn_readfirstlane( tid >> 6 );
			const int n0 = blockIdx.x * 16 * CT;
			const int m0 = SPLIT ? 0 : blockIdx.y * 16 * MT;
			const int kOff = SPLIT ? blockIdx.y * ( a.K / ( SPLIT ? SPLIT : 1 ) ) : 0;	 // first K element of this workgroup's share
			const int nk = SPLIT ? a.K / ( SPLIT ? SPLIT : 1 ) / 64 : a.K / 64, perQ = SPLIT ? nk : nk / 4, nSlots = nk / KS;
			const f16* const Ak = a.A + kOff;
			const f16* const Wk = a.W + kOff;

			// ---- producer: A = 2 MT pieces of 8 rows (wave w: pieces AP w .. AP w + AP - 1), W = 2 CT pieces (CT = 4: 2 w, 2 w + 1; CT = 2: piece w)
			const int rIn = lane >> 3, cPhys = lane & 7;
			unsigned offA[ AP ], offW[ 2 ];
	#pragma unroll
			for( int i = 0; i < AP; i++ )
			{
				const int row = ( wave * AP + i ) * 8 + rIn;
				const int cl = cPhys ^ ( ( row >> 1 ) & 7 );
				int m = m0 + row;
				m = m < a.M ? m : a.M - 1;
				offA[ i ] = (unsigned)( ( rowOffset( m, a.Mb, a.lda, a.aBatchStride ) + cl * 8 ) * 2 );
			}
	#pragma unroll
			for( int i = 0; i < 2; i++ )
			{
				const int rowW = CT == 4 ? ( wave * 2 + i ) * 8 + rIn : wave * 8 + rIn;
				const int clW = cPhys ^ ( ( rowW >> 1 ) & 7 );
				int n = n0 + rowW;
				n = n < a.N ? n : a.N - 1;
				offW[ i ] = (unsigned)( ( (long long)n * a.K + clW * 8 ) * 2 );
			}
			const unsigned ldsBase = __builtin_amdgcn_readfirstlane( (unsigned)(size_t)(LdsPtr)smemD );
			auto issue = [ & ]( int slot )
			{
	#pragma unroll
				for( int u = 0; u < KS; u++ )
				{
					const int kt = slot * KS + u;
					const unsigned buf = ldsBase + (unsigned)( slot % NBUF ) * STAGE + u * TILE;
					ldsDmaPair( Ak + kt * 64, offA[ 0 ], offA[ 1 ], buf + (unsigned)wave * ( AP * 1024u ) );
					if constexpr( AP == 3 ) ldsDmaOne( Ak + kt * 64, offA[ 2 ], buf + (unsigned)wave * ( AP * 1024u ) + 2048u );
					if constexpr( AP == 4 ) ldsDmaPair( Ak + kt * 64, offA[ 2 ], offA[ 3 ], buf + (unsigned)wave * ( AP * 1024u ) + 2048u );
					if constexpr( CT == 4 )
						ldsDmaPair( Wk + kt * 64, offW[ 0 ], offW[ 1 ], buf + A_BYTES + (unsigned)wave * 2048u );
					else
						ldsDmaOne( Wk + kt * 64, offW[ 0 ], buf + A_BYTES + (unsigned)wave * 1024u );
				}
			};

			// ---- consumer: lane l reads row l & 15 of a 16-row tile, logical chunk 4 h + (l >> 4), stored at chunk ^ ((row >> 1) & 7)
			const int cTile = wave % CT, tFirst = wave / CT;	 // group g = wave + 4 i: column tile g % CT = cTile, row tile g / CT = tFirst + ( 4 / CT ) i (G = MT CT is a multiple of 4)
			unsigned fragOff[ 2 ];
	#pragma unroll
			for( int h = 0; h < 2; h++ ) fragOff[ h ] = (unsigned)( ( lane & 15 ) * 128 + ( ( ( ( h << 2 ) + ( lane >> 4 ) ) ^ ( ( lane >> 1 ) & 7 ) ) << 4 ) );

			f32x4 acc[ GPW ], tot[ GPW ];
	#pragma unroll
			for( int i = 0; i < GPW; i++ ) acc[ i ] = tot[ i ] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };

	#pragma unroll
			for( int d = 0; d < NBUF - 1; d++ )
				if( d < nSlots ) issue( d );
			int inQ = 0, quarter = 0;
			for( int slot = 0; slot < nSlots; slot++ )
			{
				// slot `slot` has landed when no more than the pieces of the (up to NBUF - 2) younger slots are outstanding
				const int younger = min( NBUF - 2, nSlots - 1 - slot );
				static_assert( NBUF == 3 || NBUF == 4, "one or two younger slots" );
				if( younger >= 2 )
					asm volatile( "s_waitcnt vmcnt(%0)" ::"n"( 2 * P ) : "memory" );
				else if( younger == 1 )
					asm volatile( "s_waitcnt vmcnt(%0)" ::"n"( P ) : "memory" );
				else
					asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
				asm volatile( "s_barrier" ::: "memory" );	 // the slot is complete for every wave; every wave has issued the MFMAs of the slot before, whose buffer the next issue overwrites
				if( slot + NBUF - 1 < nSlots ) issue( slot + NBUF - 1 );
	#pragma unroll
				for( int u = 0; u < KS; u++ )
				{
					const unsigned char* const buf = smemD + ( slot % NBUF ) * STAGE + u * TILE;
					f16x8 fw[ 2 ], fx[ GPW ][ 2 ];
	#pragma unroll
					for( int h = 0; h < 2; h++ )
					{
						fw[ h ] = *(const f16x8*)( buf + A_BYTES + cTile * 2048 + fragOff[ h ] );
	#pragma unroll
						for( int i = 0; i < GPW; i++ ) fx[ i ][ h ] = *(const f16x8*)( buf + ( tFirst + ( 4 / CT ) * i ) * 2048 + fragOff[ h ] );
					}
	#pragma unroll
					for( int h = 0; h < 2; h++ )
	#pragma unroll
						for( int i = 0; i < GPW; i++ ) acc[ i ] = __builtin_amdgcn_mfma_f32_16x16x32_f16( fw[ h ], fx[ i ][ h ], acc[ i ], 0, 0, 0 );
					if( ++inQ == perQ )
					{
						// a quarter of K is complete: the partial tile of gemvFused's wave `quarter`
	#pragma unroll
						for( int i = 0; i < GPW; i++ )
						{
	#pragma unroll
							for( int r = 0; r < 4; r++ ) tot[ i ][ r ] = quarter == 0 ? acc[ i ][ r ] : tot[ i ][ r ] + acc[ i ][ r ];
							acc[ i ] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
						}
						inQ = 0;
						quarter++;
					}
				}
			}
			if constexpr( SPLIT != 0 )
			{
				// the partial tile of this eighth of K: group g = wave + 4 i, lane = (activation row, four consecutive columns) as in decRowsEpilogue
				float* const part = a.splitScratch + (long long)blockIdx.y * a.M * a.N;
	#pragma unroll
				for( int i = 0; i < GPW; i++ )
				{
					const int g = wave + NW * i;
					const int t = g / CT, c = g - t * CT;
					const int mm = t * 16 + ( lane & 15 );
					const int nn = n0 + c * 16 + ( lane >> 4 ) * 4;
					if( mm < a.M && nn < a.N ) *(f32x4*)( part + (long long)mm * a.N + nn ) = tot[ i ];
				}
			}
			else
				decRowsEpilogue<EPI, MT, CT, NW>( a, tot, m0, n0, wave, lane );
		}

		// out[m][n] = ( ( ( P0 + P1 ) + ... + P7 ) + bias ) + res: the eight partial tiles of gemmDecTile<.., SPLIT = 8> in gemvFused's wave order, then epilogueOne<EPI_F32>'s order
		template<int SPLIT>
		__global__ void __launch_bounds__( 256 ) decSplitCombine( const GemmArgs a )
		{
			const int n4 = a.N >> 2;
			const int idx = blockIdx.x * 256 + threadIdx.x;
			if( idx >= a.M * n4 ) return;
			const int mm = idx / n4, nn = ( idx - mm * n4 ) * 4;
			const long long stride = (long long)a.M * a.N;
			const float* const p = a.splitScratch + (long long)mm * a.N + nn;
			f32x4 v[ SPLIT ];
	#pragma unroll
			for( int e = 0; e < SPLIT; e++ ) v[ e ] = *(const f32x4*)( p + e * stride );
			const long long off = (long long)mm * a.ldc + nn;
			f32x4 bv = { 0.0f, 0.0f, 0.0f, 0.0f }, rv = { 0.0f, 0.0f, 0.0f, 0.0f };
			if( a.bias ) bv = *(const f32x4*)( a.bias + nn );
			if( a.res ) rv = *(const f32x4*)( a.res + off );
			f32x4 o = v[ 0 ];
	#pragma unroll
			for( int e = 1; e < SPLIT; e++ )
	#pragma unroll
				for( int r = 0; r < 4; r++ ) o[ r ] += v[ e ][ r ];
			// (gemvFused adds its zero-initialised bias / residual registers when the pointers are null: so does this)
	#pragma unroll
			for( int r = 0; r < 4; r++ ) o[ r ] = ( o[ r ] + bv[ r ] ) + rv[ r ];
			*(f32x4*)( a.out32 + off ) = o;
		}
	}	// namespace

	// Calls f( RowTiles<MT>{} ) for the MT row tiles of 16 that hold M rows (33 .. 128 of them): 3 .. 8, or with EVEN the next of 4 / 6 / 8
	template<int MT>
	using RowTiles = std::integral_constant<int, MT>;
	template<bool EVEN, class F>
	static int withRowTiles( int M, F&& f )
	{
		const int mt = ( M + 15 ) / 16;
		if constexpr( !EVEN )
		{
			if( mt == 3 ) return f( RowTiles<3>{} );
			if( mt == 5 ) return f( RowTiles<5>{} );
			if( mt == 7 ) return f( RowTiles<7>{} );
		}
		if( EVEN ? mt <= 4 : mt == 4 ) return f( RowTiles<4>{} );
		if( EVEN ? mt <= 6 : mt == 6 ) return f( RowTiles<6>{} );
		return f( RowTiles<8>{} );
	}

	// 33 .. 128 rows, EPI_F32, A in global memory, at least 512 column tiles. Returns 1 when the shape is not covered.
	static int launchAllRows( const GemmArgs& a, hipStream_t stream )
	{
		const int tiles = ( a.N + 31 ) / 32;
		if( a.lnX || a.epi != EPI_F32 || a.M <= 32 || a.M > 128 || ( a.K % 128 ) != 0 || tiles < 512 ) return 1;
		return withRowTiles<false>( a.M, [ & ]( auto mtTag ) {
			constexpr int MT = decltype( mtTag )::value;
			return launchLds<gemmAllRows<EPI_F32, MT>>( dim3( tiles ), dim3( 256 ), 4 * MT * 2 * 4 * 64 * 4, stream, a );
		} );
	}

	template<int EPI, int MT, int CT, int DEPTH, int NW = 4>
	static int launchDecRowsD( const GemmArgs& a, hipStream_t stream )
	{
		return launchLds<gemmDecRows<EPI, MT, CT, DEPTH, NW>>( dim3( ( a.N + 16 * CT - 1 ) / ( 16 * CT ), ( a.M + 16 * MT - 1 ) / ( 16 * MT ) ), dim3( NW * 64 ), NW * MT * CT * 4 * 64 * 4, stream, a );
	}
	template<int EPI, int MT, int CT>
	static int launchDecRowsK( const GemmArgs& a, hipStream_t stream )
	{
		constexpr int deep = MT * CT >= 16 ? 2 : ( MT * CT >= 8 ? 3 : 4 );
		if constexpr( deep != 2 )
			if( g_opt.decDepth != 2 ) return launchDecRowsD<EPI, MT, CT, deep>( a, stream );
		return launchDecRowsD<EPI, MT, CT, 2>( a, stream );
	}

	// gemmDecTile: K must divide into four quarters of whole 64-element tiles (the K split the sums follow); operands addressed as a 64-bit base + 32-bit offsets
	// SPLIT = 8: blockIdx.y is the eighth of K instead of the row tile (all rows in the one tile of 16 MT)
	template<int EPI, int CT, int KS = 1, int NBUF = DT_NBUF, int MT = 4, int SPLIT = 0>
	static int launchDecTileK( const GemmArgs& a, hipStream_t stream )
	{
		return launchLds<gemmDecTile<EPI, CT, KS, NBUF, MT, SPLIT>>( dim3( ( a.N + 16 * CT - 1 ) / ( 16 * CT ), SPLIT ? SPLIT : ( a.M + 16 * MT - 1 ) / ( 16 * MT ) ), dim3( 256 ),
			NBUF * KS * ( MT * 16 * 128 + CT * 16 * 128 ), stream, a );
	}
	static bool decTileOk( const GemmArgs& a )
	{
		const long long aBytes = 2ll * ( a.Mb > 0 && a.Mb < a.M ? ( (long long)( a.M / a.Mb ) + 1 ) * a.aBatchStride + (long long)a.Mb * a.lda : (long long)a.M * a.lda ) + 2ll * a.K;
		return ( a.K % 256 ) == 0 && ( a.lda % 8 ) == 0 && ( a.aBatchStride % 8 ) == 0 && aBytes < ( 1ll << 31 ) && 2ll * a.N * a.K < ( 1ll << 31 );
	}

	// Tile of a big-batch decode product: 64 x 64 (rows x columns) while that leaves enough workgroups for the chip, else 64 x 32, else 32 x 32.
	// Option dec_tile = <MT><CT> (44, 42, 24, 22) pins one for A/B runs and tests.
	template<int EPI>
	static int launchDecRowsT( const GemmArgs& a, hipStream_t stream )
	{
		const int pinned = g_opt.decTile;
		auto wgs = [ & ]( int mt, int ct ) { return ( ( a.N + 16 * ct - 1 ) / ( 16 * ct ) ) * ( ( a.M + 16 * mt - 1 ) / ( 16 * mt ) ); };
		// option dec_lds: the LDS-staged kernel (64 x 64, or 64 x 32 while the wider tile leaves fewer than 192 workgroups)
		// (measured, tools/gemv_time.py: 448 x 4096 x 1024 14.4 against 22.1 us, 448 x 1024 x 4096 21.2 / 26.7, 448 x 1024 x 1024 7.7 / 9.2, 224 x 4096 x 1024 10.8 / 14.1;
		// at 224 rows the N = 1024 products would get 128 workgroups of 64 x 32 and lose to gemmDecRows' 32 x 32 tiles: 7.6 / 6.6 and 20.5 / 18.1 us -- those keep it)
		if( g_opt.decLds == 1 && pinned == 0 && decTileOk( a ) )
		{
			if( wgs( 4, 4 ) >= 192 ) return launchDecTileK<EPI, 4>( a, stream );
			// (64 x 32 tiles from 160 workgroups: 320 x 1024 x 4096 17.5 against 30.9 us, 320 x 1024 x 1024 7.6 / 10.1; at 128 workgroups -- 224 / 256 rows -- 7.6 against 6.5 us)
			if( wgs( 4, 2 ) >= 160 )
			{
				// deep products (the MLP down-projection): two K tiles per ring slot and barrier when a quarter of K is an even number of tiles (448 x 1024 x 4096: 18.1 against 21.7 us)
				if( g_opt.decLdsKs == 2 && a.K >= 2048 && ( a.K % 512 ) == 0 ) return launchDecTileK<EPI, 2, 2, 3>( a, stream );
				return launchDecTileK<EPI, 2>( a, stream );
			}
		}
		int tile = pinned;
		if( tile != 44 && tile != 42 && tile != 24 && tile != 22 )
			tile = wgs( 4, 4 ) >= 192 ? 44 : ( wgs( 4, 2 ) >= 192 ? 42 : 22 );
		switch( tile )
		{
		case 44: return launchDecRowsK<EPI, 4, 4>( a, stream );
		case 42: return launchDecRowsK<EPI, 4, 2>( a, stream );
		case 24: return launchDecRowsK<EPI, 2, 4>( a, stream );
		default: return launchDecRowsK<EPI, 2, 2>( a, stream );
		}
	}

	// 33 .. 128 rows against a WIDE weight matrix (N >= 2048: the MLP up-projection, the fused QKV product): ALL rows in one row tile of 16 MT rows and 32
	// columns per workgroup. gemvFused's 16-column workgroups re-read the rows once per 16 columns: at 70 rows and N = 4096 that is 82 MB of L2 -> CU
	// traffic for 8 MB of weights (15 us per launch); here 29 MB over N / 32 workgroups. Same K split and summation order: the same bits.
	template<int EPI>
	static int launchDecRowsOneTile( const GemmArgs& a, hipStream_t stream )
	{
		// option dec_lds (round 6): the LDS-staged kernel with all rows in one workgroup per 32 columns (4 / 6 / 8 row tiles), the same sums
		if( g_opt.decLds == 1 && g_opt.decTile == 0 && decTileOk( a ) )
		{
			// two K tiles per ring slot and barrier (dec_lds_ks 2, the default) for 4 and 6 row tiles: 40 x 5120 x 1280 8.9 -> 7.8 us, 70 rows 10.9 -> 10.0; level at 8
			// row tiles (123 KiB of LDS), and SLOWER for the K-split instances (K = 5120 at 70 rows: 11.9 -> 13.9) and the vocabulary product (38 -> 48 us: one
			// workgroup per CU instead of three) -- those keep one tile per slot (profiles/r06_evidence/small_batch_products.txt)
			const bool ks2 = g_opt.decLdsKs == 2 && ( a.K % 128 ) == 0;
			return withRowTiles<true>( a.M, [ & ]( auto mtTag ) {
				constexpr int MT = decltype( mtTag )::value;
				if constexpr( MT <= 6 )
					if( ks2 ) return launchDecTileK<EPI, 2, 2, 3, MT>( a, stream );
				return launchDecTileK<EPI, 2, 1, DT_NBUF, MT>( a, stream );
			} );
		}
		return withRowTiles<false>( a.M, [ & ]( auto mtTag ) { return launchDecRowsK<EPI, decltype( mtTag )::value, 2>( a, stream ); } );
	}
	// 33 .. 128 rows against a NARROW, DEEP weight matrix (N <= 2048, K >= 2048: the MLP down-projection): 16 columns x all rows per workgroup, EIGHT waves
	// splitting K -- gemvFused's own split for this product (TUNE_GEMV_K8), so the same bits -- instead of its 16 columns x 32 rows with the rows re-read per group
	// (loads 4 deep; 3 at 8 row tiles)
	static int launchDecRowsDeep( const GemmArgs& a, hipStream_t stream )
	{
		if( a.lnX || a.epi != EPI_F32 || a.M <= 32 || a.M > GEMV_FUSED_MAX_ROWS || a.N > 2048 || ( a.N % 16 ) != 0 || a.K < 2048 || ( a.K % 256 ) != 0 || !( g_tuning & TUNE_GEMV_K8 ) ) return 1;
		return withRowTiles<false>( a.M, [ & ]( auto mtTag ) {
			constexpr int MT = decltype( mtTag )::value;
			return launchDecRowsD<EPI_F32, MT, 1, MT == 8 ? 3 : 4, 8>( a, stream );
		} );
	}
	// 33 .. 128 rows against a NARROW, DEEP weight matrix, option dec_split (round 6): the eight K shares of gemvFused's eight waves dealt to eight workgroups of the
	// LDS-staged kernel per 32 columns (N / 32 x 8 = 256 .. 320 workgroups instead of gemvFused's N / 16 x 2 re-reading the rows per 16 columns), the eight partial tiles
	// added by a second launch in wave order: the same bits. Needs the context's scratch (8 x M x N floats). Returns 1 when the shape is not covered.
	static bool decSplitShape( const GemmArgs& a )
	{
		// (measured and not kept: LayerNorm of the finished rows for the next product inside the combine launch, a wave per row -- 10 workgroups at 40 rows take 6.2 us
		// against 2.5 + 5.3 for the two launches it replaces, the beam job did not move: 1271 against 1270 audio-s/s)
		return !( a.lnX || a.epi != EPI_F32 || !a.splitScratch || a.M <= 32 || a.M > GEMV_FUSED_MAX_ROWS || a.N > 2048 || ( a.N % 32 ) != 0 || a.K < 2048 || ( a.K % 512 ) != 0 || a.Mb < a.M ||
			!( g_tuning & TUNE_GEMV_K8 ) || !decTileOk( a ) );
	}
	static int launchDecRowsSplit( const GemmArgs& a, hipStream_t stream )
	{
		if( !decSplitShape( a ) ) return 1;
		WH_CHECK( withRowTiles<true>( a.M, [ & ]( auto mtTag ) { return launchDecTileK<EPI_F32, 2, 1, DT_NBUF, decltype( mtTag )::value, 8>( a, stream ); } ) );
		return launchLds<decSplitCombine<8>>( dim3( ( a.M * ( a.N / 4 ) + 255 ) / 256 ), dim3( 256 ), 0, stream, a );
	}
	// returns 1 when the shape is not one of these
	static int launchDecRowsWide( const GemmArgs& a, hipStream_t stream )
	{
		if( a.lnX || a.M <= 32 || a.M > GEMV_FUSED_MAX_ROWS || a.N < 2048 || ( a.K % 128 ) != 0 || a.K > 2048 ) return 1;
		switch( a.epi )
		{
		case EPI_F16_GELU: return launchDecRowsOneTile<EPI_F16_GELU>( a, stream );
		case EPI_QKV_DEC: return launchDecRowsOneTile<EPI_QKV_DEC>( a, stream );
		case EPI_F32: if( g_opt.decWideRows == 2 ) return launchDecRowsOneTile<EPI_F32>( a, stream ); break;	 // (diagnostic: the accumulators of the one-tile instances in FP32)
		}
		return 1;
	}

	// 129 .. GEMV_MAX_ROWS rows, A in global memory (a LayerNorm in front is its own launch at this many rows)
	static int launchDecRows( const GemmArgs& a, hipStream_t stream )
	{
		if( a.lnX || ( a.K % 128 ) != 0 )
		{
			setError( "gemv: more than 128 rows need FP16 activation rows and K a multiple of 128" );
			return -1;
		}
		switch( a.epi )
		{
		case EPI_F32: return launchDecRowsT<EPI_F32>( a, stream );
		case EPI_F16_GELU: return launchDecRowsT<EPI_F16_GELU>( a, stream );
		case EPI_QKV_DEC: return launchDecRowsT<EPI_QKV_DEC>( a, stream );
		case EPI_Q_DEC: return launchDecRowsT<EPI_Q_DEC>( a, stream );
		}
		setError( "gemv: epilogue not available" );
		return -1;
	}

	template<int EPI, int PRO, int ROWS, int NW, int UNROLL, int MT>
	static int launchGemvK( const GemmArgs& a, hipStream_t stream )
	{
		const size_t lds = PRO != 0 ? (size_t)16 * MT * GV_XS_STRIDE * sizeof( f16 ) : 0;
		const int groups = ( a.M + 16 * MT - 1 ) / ( 16 * MT );
		return launchLds<gemvFused<EPI, PRO, ROWS, NW, UNROLL, MT>>( dim3( ( a.N + ROWS - 1 ) / ROWS, groups ), dim3( NW * 64 ), lds, stream, a );
	}

	template<int EPI, int PRO, int ROWS = 16, int NW = 4>
	static int launchGemvT( const GemmArgs& a, hipStream_t stream )
	{
		// a wave holds K / NW / 32 weight fragments; when they fit in 8 slots the 8-slot instance does the same work with
		// half the registers, which lets kernels of concurrent decode chains share a CU. More than 16 activation rows
		// (up to 32) take a second MFMA column tile per weight fragment.
		const bool small = a.K / NW / 32 <= 8 && ( g_tuning & TUNE_GEMV_SMALLREG );
		if constexpr( PRO == 0 )
		{
			// 33 .. 128 rows: four MFMA column tiles per weight fragment (64 rows per workgroup, two row groups beyond that);
			// always the 8-slot instance -- 4 x 8 activation fragments in flight are 128 registers
			if( a.M > 32 )
			{
				// 64 rows per workgroup read each weight row once per 64 rows, but N / ROWS x ceil(M / 64) workgroups must still
				// cover the chip: below 256 of them, 32 rows per workgroup (twice the workgroups, each with half the activation
				// traffic) measured 5.8 vs 7.8 us (N = K = 1024) and 14.1 vs 22.0 us (N = 1024, K = 4096) at 112 rows
				// TUNE_GEMV_MT8 (A/B): ALL rows in one workgroup when N / ROWS alone fills the chip (the MLP up-projection, N = 4096): the weights are
				// streamed once instead of once per 64 rows; 4 fragment slots instead of 8 keep 8 x 4 activation fragments at 128 registers
				if constexpr( NW == 4 )
					if( a.M > 64 && ( a.N + ROWS - 1 ) / ROWS >= 256 && ( g_tuning & TUNE_GEMV_MT8 ) ) return launchGemvK<EPI, PRO, ROWS, NW, 4, 8>( a, stream );
				const int wgs = ( a.N + ROWS - 1 ) / ROWS * ( ( a.M + 63 ) / 64 );
				if( wgs < 256 && ( g_tuning & TUNE_GEMV_ROWGROUPS ) ) return launchGemvK<EPI, PRO, ROWS, NW, 8, 2>( a, stream );
				return launchGemvK<EPI, PRO, ROWS, NW, 8, 4>( a, stream );
			}
		}
		if( a.M > 16 )
			return small ? launchGemvK<EPI, PRO, ROWS, NW, 8, 2>( a, stream ) : launchGemvK<EPI, PRO, ROWS, NW, GV_UNROLL_MAX, 2>( a, stream );
		return small ? launchGemvK<EPI, PRO, ROWS, NW, 8, 1>( a, stream ) : launchGemvK<EPI, PRO, ROWS, NW, GV_UNROLL_MAX, 1>( a, stream );
	}

	int launchGemv( const GemmArgs& a, hipStream_t stream )
	{
		if( a.M <= 0 || a.M > GEMV_MAX_ROWS || a.N <= 0 || a.K <= 0 || ( a.K % 128 ) != 0 )
		{
			setError( "gemv: need 0 < M <= 512 and K a multiple of 128" );
			return -1;
		}
		// more than 128 rows (a lock-step batch of 129 .. 512 sequences): 64 x 64 output tiles per workgroup (gemmDecRows).
		// Option dec_tile = 1 keeps gemvFused (16 columns x 64 rows per workgroup, row groups in blockIdx.y) for A/B runs.
		if( a.M > GEMV_FUSED_MAX_ROWS && ( g_opt.decTile != 1 || a.lnX ) ) return launchDecRows( a, stream );
		const bool ln = a.lnX != nullptr;
		// option dec_wide_rows: 33 .. 128 rows against N >= 2048 in one row tile per 32 columns (gemmDecRows) instead of gemvFused's 16-column workgroups
		if( a.M > 32 && !ln && g_opt.decWideRows )
		{
			const int rc = launchDecRowsWide( a, stream );
			if( rc <= 0 ) return rc;
		}
		// option dec_split: the same product with the eight K shares on eight workgroups of gemmDecTile and a combine launch
		if( a.M > 32 && !ln && g_opt.decSplit )
		{
			const int rc = launchDecRowsSplit( a, stream );
			if( rc <= 0 ) return rc;
		}
		// option dec_deep_rows: 33 .. 128 rows against N <= 2048, K >= 2048 (MLP down-projection) with all rows per 16-column workgroup and 8 waves over K
		if( a.M > 32 && !ln && g_opt.decDeepRows )
		{
			const int rc = launchDecRowsDeep( a, stream );
			if( rc <= 0 ) return rc;
		}
		// option vocab_lds (round 6): the vocabulary product (N / 32 >= 512) of 33 .. 128 rows as 64 x 64 tiles of the LDS-staged kernel (one or two row tiles): the rows
		// are re-read once per 64 columns instead of gemmAllRows' once per 32, the second row tile finds the weights in the Infinity Cache; the same K quarters added in
		// the same order (40 x 51865 x 1280: 37.7 against 67.1 us, 128 rows: 67.7 against 132.8)
		if( a.M > 32 && a.M <= GEMV_FUSED_MAX_ROWS && !ln && a.epi == EPI_F32 && ( a.N + 31 ) / 32 >= 512 && a.Mb >= a.M && g_opt.vocabLds == 1 && ( g_tuning & TUNE_GEMV_ALLROWS ) && decTileOk( a ) )
			return launchDecTileK<EPI_F32, 4>( a, stream );
		if( a.M > 32 && !ln && ( g_tuning & TUNE_GEMV_ALLROWS ) )
		{
			const int rc = launchAllRows( a, stream );
			if( rc <= 0 ) return rc;
		}
		if( ln && ( a.K > GV_MAXK_LN || a.M > 32 ) )
		{
			setError( "gemv: the fused LayerNorm prologue supports up to 32 rows of up to 1280 columns" );
			return -1;
		}
		// small N, large K (the MLP down projection): 4 weight rows per workgroup so that every CU streams
		// (up to 16 activation rows: beyond that the rows a workgroup re-reads outweigh its 4 weight rows, measured +3 % without)
		const bool rows4 = !ln && a.epi == EPI_F32 && ( a.N % 16 ) == 0 && a.N <= 2048 && a.K >= 2048 && a.M <= 16 && ( g_tuning & TUNE_GEMV_ROWS4 );
		// K >= 2048 (the MLP down-projection, 64 workgroups): 8 waves split K, so a wave's 16 weight fragments are ONE round of loads
		const bool k8 = !ln && !rows4 && a.epi == EPI_F32 && a.K >= 2048 && ( a.K % 256 ) == 0 && ( g_tuning & TUNE_GEMV_K8 );
		// more than 16 rows: the LayerNorm prologue is done by the whole workgroup, 16 rows at a time
		const bool lnBlock = ln && a.M > 16;
		switch( a.epi )
		{
		case EPI_F32:
			if( lnBlock ) return launchGemvK<EPI_F32, 2, 16, 4, 8, 2>( a, stream );
			if( ln ) return launchGemvT<EPI_F32, 1>( a, stream );
			if( k8 ) return launchGemvT<EPI_F32, 0, 16, 8>( a, stream );
			return rows4 ? launchGemvT<EPI_F32, 0, 4, 4>( a, stream ) : launchGemvT<EPI_F32, 0>( a, stream );
		case EPI_F16_GELU:
			if( lnBlock ) return launchGemvK<EPI_F16_GELU, 2, 16, 4, 8, 2>( a, stream );
			return ln ? launchGemvT<EPI_F16_GELU, 1>( a, stream ) : launchGemvT<EPI_F16_GELU, 0>( a, stream );
		case EPI_QKV_DEC:
			if( lnBlock ) return launchGemvK<EPI_QKV_DEC, 2, 16, 4, 8, 2>( a, stream );
			return ln ? launchGemvT<EPI_QKV_DEC, 1>( a, stream ) : launchGemvT<EPI_QKV_DEC, 0>( a, stream );
		case EPI_Q_DEC:
			if( lnBlock ) return launchGemvK<EPI_Q_DEC, 2, 16, 4, 8, 2>( a, stream );
			return ln ? launchGemvT<EPI_Q_DEC, 1>( a, stream ) : launchGemvT<EPI_Q_DEC, 0>( a, stream );
		}
		setError( "gemv: epilogue not available" );
		return -1;
	}

	int launchGemmSkinny( const GemmArgs& a, hipStream_t stream )
	{
		if( a.M > 32 )
			return launchGemm( a, stream );
		WH_CHECK( checkGemmArgs( a ) );
		const dim3 grid( ( a.N + 31 ) / 32 ), block( 256 );
		switch( a.epi )
		{
		case EPI_F32: return launchLds<gemmSkinny<EPI_F32>>( grid, block, 0, stream, a );
		case EPI_F16_GELU: return launchLds<gemmSkinny<EPI_F16_GELU>>( grid, block, 0, stream, a );
		case EPI_QKV_DEC: return launchLds<gemmSkinny<EPI_QKV_DEC>>( grid, block, 0, stream, a );
		case EPI_Q_DEC: return launchLds<gemmSkinny<EPI_Q_DEC>>( grid, block, 0, stream, a );
		}
		setError( "gemm: epilogue not available in the skinny kernel" );
		return -1;
	}
}
