// gemvW8: the decode-step product for INT8 decoder weights ("INT8 decoder weights"; wh_context_set_decoder_w8).
//
//   out[m][n] = epilogue( ( sum_k x[m][k] * (float)q[n][k] ) * sw[n] )
//
// q int8 [N][K] with one FP32 scale per weight row (quantizeRowsI8's format: s = amax / 127, q = rint( x / s ) in [-127, 127]), x FP16 rows or the fused LayerNorm
// prologue of gemvFused (a wave per pair of rows up to 16 rows, the whole workgroup up to 32), 1 .. 128 activation rows, K a multiple of 128 up to 5120, any N.
// Weights only are quantized: an int8 value is exact in FP16, so x * q is exact on v_mfma_f32_16x16x32_f16, the sum is FP32 and the row scale is applied once, to
// the sum. Against the float64 product of the same int8 weights only the summation order differs.
//
// The kernel is latency- and HBM-bound like gemvFused (gemm_decode.hip); what it is built around is the int8 row:
//   * a lane's 16-byte weight load holds SIXTEEN k-values of one weight row, twice an FP16 fragment, and feeds TWO MFMAs: bytes 0 .. 7 are the A operand of the first,
//     bytes 8 .. 15 of the second. A wave's k-step is therefore 64 wide (4 lane groups x 16), and lane group g reads the activations at the matching positions,
//     x[ k0 + 16 g .. + 15 ], as two 16-byte fragments: the sum over k does not care how k is dealt to the operand slots as long as both operands agree.
//   * every weight load of a wave (up to 8 slots = 512 k-values; 10 slots for the eight-wave split, which is all of K <= 5120) is requested non-temporally before
//     the prologue, the epilogue operands or anything else.
//   * NW waves split K: 8 when K >= 2048 and K / 8 is whole k-steps (the MLP down-projection: a wave's share is one round of loads), 4 when K / 4 is, else 2.
//   * ROWS weight rows per workgroup: 16 fill the MFMA's row slots; 4 (each row in four slots, the loads of the four coalesce) while N / 16 workgroups would leave
//     CUs without a workgroup (N = 1024: 256 workgroups instead of 64) -- FP32 epilogue, FP16 rows, up to 32 activation rows.
//   * MT column tiles of 16 activation rows per weight fragment: 1, 2 or 4, further row groups in blockIdx.y (gemvFused's range and rule: 32 rows per workgroup
//     while 64 would leave fewer than 256 workgroups).
//   * int8 -> FP16 in registers, per dword of four bytes: v_xor_b32 with 0x80808080 (b + 128 as an unsigned byte), two v_perm_b32 that put each byte under the
//     constant 0x64 (the half 0x6400 | u is 1024 + u exactly), two v_pk_add_f16 of -1152: FIVE instructions per 4 bytes, TWENTY per 16-byte load and pair of MFMAs,
//     all exact. Plain converts (v_cvt_f32_i32 on an SDWA byte, v_cvt_pkrtz_f16_f32) take six per dword.
//   * the partial tiles of the waves meet in LDS and wave 0 adds them in wave order 1, 2, ..: two launches give the same bits.
// Plain C++ and builtins; no inline assembly.
#include "gemm_device.h"
#include "gemm_launch.h"

namespace wh
{
	namespace
	{
		// sixteen int8 -> the two FP16 A fragments of a pair of MFMAs (k-values 0 .. 7 and 8 .. 15 of the load)
		__device__ __forceinline__ void w8Fragments( const u32x4 w, f16x8& lo, f16x8& hi )
		{
			const f16x2 off = { (f16)1152.0f, (f16)1152.0f };
			unsigned h[ 8 ];
	#pragma unroll
			for( int i = 0; i < 4; i++ )
			{
				const unsigned x = w[ i ] ^ 0x80808080u;
				// v_perm_b32: selector bytes 4 .. 7 take bytes 0 .. 3 of the first operand, 0 .. 3 those of the second
				const unsigned p0 = __builtin_amdgcn_perm( x, 0x64646464u, 0x00050004u );
				const unsigned p1 = __builtin_amdgcn_perm( x, 0x64646464u, 0x00070006u );
				h[ 2 * i ] = __builtin_bit_cast( unsigned, __builtin_bit_cast( f16x2, p0 ) - off );
				h[ 2 * i + 1 ] = __builtin_bit_cast( unsigned, __builtin_bit_cast( f16x2, p1 ) - off );
			}
			lo = __builtin_bit_cast( f16x8, u32x4{ h[ 0 ], h[ 1 ], h[ 2 ], h[ 3 ] } );
			hi = __builtin_bit_cast( f16x8, u32x4{ h[ 4 ], h[ 5 ], h[ 6 ], h[ 7 ] } );
		}

		// PRO = 0: A rows are FP16 in global memory; 1: LayerNorm prologue, a wave per pair of rows (up to 16 rows, MT = 1); 2: by the whole workgroup (17 .. 32 rows, MT = 2)
		template<int EPI, int PRO, int ROWS, int NW, int MT>
		__global__ void __launch_bounds__( NW * 64 ) gemvW8( const GemvW8Args p )
		{
			const GemmArgs& a = p.g;
			constexpr int UN = NW == 8 ? 10 : 8;	 // weight slots of a wave
			constexpr int XB = MT == 1 ? 8 : 4;		 // k-steps whose activation fragments (2 MT per step) are requested together
			constexpr int RB = NW >= 4 ? 16 : 8;	 // PRO 2: rows the workgroup normalises at a time (two waves hold three float4 columns of a row each)
			__shared__ float red[ NW - 1 ][ MT * 4 ][ 64 ];
			__shared__ float lnA[ PRO == 2 ? NW : 1 ][ RB ], lnB2[ PRO == 2 ? NW : 1 ][ RB ];
			extern __shared__ __attribute__( ( aligned( 16 ) ) ) f16 xs[];	 // [16 * MT][GV_XS_STRIDE] when there is a prologue

			const int tid = threadIdx.x;
			const int lane = tid & 63;
			const int wave = tid >> 6;
			const int n0 = blockIdx.x * ROWS;
			const int m0 = blockIdx.y * 16 * MT;
			const int mEnd = a.M;

			int n = n0 + ( lane & 15 ) % ROWS;
			n = n < a.N ? n : a.N - 1;	   // the last workgroup clamps: the rows beyond N are never stored
			const int kPer = a.K / NW;
			const int kBeg = wave * kPer + ( lane >> 4 ) * 16;
			const int8_t* const pw = p.W8 + (long long)n * a.K + kBeg;
			const int steps = kPer / 64;

			u32x4 fw[ UN ];
	#pragma unroll
			for( int u = 0; u < UN; u++ )
				if( u < steps ) fw[ u ] = __builtin_nontemporal_load( (const u32x4*)( pw + u * 64 ) );

			// wave 0 owns the epilogue: its row scales, and the operands of the vector epilogues, are fetched up front as well
			const int nEp = n0 + ( lane >> 4 ) * 4;
			const bool ownsRows = ( lane >> 4 ) * 4 < ROWS && nEp < a.N;	   // with ROWS == 4 only the first 16 lanes hold distinct output rows
			const bool vec = p.vecEpi != 0;
			f32x4 swv = { 0.0f, 0.0f, 0.0f, 0.0f }, biasv = { 0.0f, 0.0f, 0.0f, 0.0f }, resv[ MT ];
	#pragma unroll
			for( int t = 0; t < MT; t++ ) resv[ t ] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
			if( wave == 0 && ownsRows )
			{
	#pragma unroll
				for( int r = 0; r < 4; r++ ) swv[ r ] = p.sw[ nEp + r < a.N ? nEp + r : a.N - 1 ];
				if( vec && ( EPI == EPI_F32 || EPI == EPI_F16_GELU ) )
				{
					if( a.bias ) biasv = *(const f32x4*)( a.bias + nEp );
					if constexpr( EPI == EPI_F32 )
					{
	#pragma unroll
						for( int t = 0; t < MT; t++ )
							if( a.res && m0 + t * 16 + ( lane & 15 ) < mEnd ) resv[ t ] = *(const f32x4*)( a.res + (long long)( m0 + t * 16 + ( lane & 15 ) ) * a.ldc + nEp );
					}
				}
			}

			if constexpr( PRO == 1 )
			{
				// rows wave and wave + NW together, then the next pair. Rows at or beyond M stay unwritten: an MFMA output column depends on its own activation
				// row only, and those columns are never stored.
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
				for( int r0 = 0; r0 < a.M; r0 += RB )
					layerNormBlock<RB, ( GV_MAXK_LN / 4 + NW * 64 - 1 ) / ( NW * 64 ), NW>( a.lnX + (long long)r0 * a.K, a.M - r0, a.lnW, a.lnB, a.K, tid, lnA, lnB2,
						[ = ]( int j, int c, f16x4 v ) { *(f16x4*)( xs + ( r0 + j ) * GV_XS_STRIDE + c ) = v; } );
				__syncthreads();
			}
			const f16* px[ MT ];
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
			for( int s0 = 0; s0 < steps; s0 += UN )
			{
				if( s0 > 0 )
				{
	#pragma unroll
					for( int u = 0; u < UN; u++ )
						if( s0 + u < steps ) fw[ u ] = __builtin_nontemporal_load( (const u32x4*)( pw + ( s0 + u ) * 64 ) );
				}
	#pragma unroll
				for( int ub = 0; ub < UN; ub += XB )
				{
					f16x8 fx[ XB ][ MT ][ 2 ];
	#pragma unroll
					for( int j = 0; j < XB; j++ )
						if( ub + j < UN && s0 + ub + j < steps )
						{
	#pragma unroll
							for( int t = 0; t < MT; t++ )
							{
								const f16* const q = px[ t ] + ( s0 + ub + j ) * 64;
								fx[ j ][ t ][ 0 ] = *(const f16x8*)q;
								fx[ j ][ t ][ 1 ] = *(const f16x8*)( q + 8 );
							}
						}
	#pragma unroll
					for( int j = 0; j < XB; j++ )
						if( ub + j < UN && s0 + ub + j < steps )
						{
							f16x8 lo, hi;
							w8Fragments( fw[ ub + j < UN ? ub + j : 0 ], lo, hi );
	#pragma unroll
							for( int t = 0; t < MT; t++ )
							{
								acc[ t ] = __builtin_amdgcn_mfma_f32_16x16x32_f16( lo, fx[ j ][ t ][ 0 ], acc[ t ], 0, 0, 0 );
								acc[ t ] = __builtin_amdgcn_mfma_f32_16x16x32_f16( hi, fx[ j ][ t ][ 1 ], acc[ t ], 0, 0, 0 );
							}
						}
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

			// D[row][col]: col = lane & 15 = activation row within the tile, row = (lane >> 4) * 4 + r = weight row slot. The row scale, once, on the FP32 sum.
			if( !ownsRows ) return;
	#pragma unroll
			for( int t = 0; t < MT; t++ )
			{
				const int mm = m0 + t * 16 + ( lane & 15 );
				if( mm >= mEnd ) continue;
				f32x4 y;
	#pragma unroll
				for( int r = 0; r < 4; r++ ) y[ r ] = __fmul_rn( acc[ t ][ r ], swv[ r ] );
				if( vec && EPI == EPI_F32 )
				{
					// out = (y + bias) + res, the same order as epilogueOne<EPI_F32>
					f32x4 o;
	#pragma unroll
					for( int r = 0; r < 4; r++ ) o[ r ] = ( y[ r ] + biasv[ r ] ) + resv[ t ][ r ];
					*(f32x4*)( a.out32 + (long long)mm * a.ldc + nEp ) = o;
					continue;
				}
				if( vec && EPI == EPI_F16_GELU )
				{
					// gelu16( y + bias ), the arithmetic of epilogueOne<EPI_F16_GELU>, four columns as one 8-byte store
					f16x4 hv;
	#pragma unroll
					for( int r = 0; r < 4; r++ ) hv[ r ] = gelu16( y[ r ] + biasv[ r ] );
					*(f16x4*)( a.out16 + (long long)mm * a.ldc + nEp ) = hv;
					continue;
				}
	#pragma unroll
				for( int r = 0; r < 4; r++ )
					if( nEp + r < a.N ) epilogueOne<EPI>( a, mm, nEp + r, y[ r ] );
			}
		}
	}	// namespace

	template<int EPI, int PRO, int ROWS, int NW, int MT>
	static int launchW8K( const GemvW8Args& a, hipStream_t stream )
	{
		const size_t lds = PRO != 0 ? (size_t)16 * MT * GV_XS_STRIDE * sizeof( f16 ) : 0;
		const int groups = ( a.g.M + 16 * MT - 1 ) / ( 16 * MT );
		return launchLds<gemvW8<EPI, PRO, ROWS, NW, MT>>( dim3( ( a.g.N + ROWS - 1 ) / ROWS, groups ), dim3( NW * 64 ), lds, stream, a );
	}
	// the K split: 8 waves when K >= 2048 and an eighth of K is whole k-steps of 64, 4 when a quarter is, else 2 (K is a multiple of 128). A prologue (K <= 1280) has 2 or 4.
	template<int EPI, int PRO, int ROWS, int MT>
	static int launchW8N( const GemvW8Args& a, hipStream_t stream )
	{
		const int K = a.g.K;
		if constexpr( PRO == 0 )
			if( K >= 2048 && ( K % 512 ) == 0 ) return launchW8K<EPI, PRO, ROWS, 8, MT>( a, stream );
		if( ( K % 256 ) == 0 ) return launchW8K<EPI, PRO, ROWS, 4, MT>( a, stream );
		return launchW8K<EPI, PRO, ROWS, 2, MT>( a, stream );
	}
	template<int EPI>
	static int launchW8E( const GemvW8Args& a, hipStream_t stream )
	{
		const GemmArgs& g = a.g;
		if( g.lnX ) return g.M <= 16 ? launchW8N<EPI, 1, 16, 1>( a, stream ) : launchW8N<EPI, 2, 16, 2>( a, stream );
		const int wgs16 = ( g.N + 15 ) / 16;
		if( g.M <= 32 )
		{
			// 4 weight rows per workgroup while 16 would leave CUs idle (N = 1024: 256 workgroups instead of 64)
			if constexpr( EPI == EPI_F32 )
				if( wgs16 < 256 && ( g.N % 4 ) == 0 ) return g.M <= 16 ? launchW8N<EPI, 0, 4, 1>( a, stream ) : launchW8N<EPI, 0, 4, 2>( a, stream );
			return g.M <= 16 ? launchW8N<EPI, 0, 16, 1>( a, stream ) : launchW8N<EPI, 0, 16, 2>( a, stream );
		}
		// 33 .. 128 rows: 64 rows per workgroup read each weight row once per 64 rows; 32 while that leaves fewer than 256 workgroups (gemvFused's rule)
		if( wgs16 * ( ( g.M + 63 ) / 64 ) < 256 ) return launchW8N<EPI, 0, 16, 2>( a, stream );
		return launchW8N<EPI, 0, 16, 4>( a, stream );
	}

	int launchGemvW8( const GemvW8Args& in, hipStream_t stream )
	{
		GemvW8Args a = in;
		const GemmArgs& g = a.g;
		if( !a.W8 || !a.sw || ( !g.lnX && !g.A ) || ( g.lnX && ( !g.lnW || !g.lnB ) ) )
		{
			setError( "gemvW8: null operand (int8 weights, row scales, and FP16 rows or the three LayerNorm operands)" );
			return -1;
		}
		if( g.M <= 0 || g.M > GEMV_W8_MAX_ROWS || g.N <= 0 || g.K <= 0 || ( g.K % 128 ) != 0 || g.K > 5120 )
		{
			setError( "gemvW8: need 0 < M <= 128 and K a multiple of 128, at most 5120" );
			return -1;
		}
		if( g.lnX && ( g.K > GV_MAXK_LN || g.M > 32 ) )
		{
			setError( "gemvW8: the fused LayerNorm prologue supports up to 32 rows of up to 1280 columns" );
			return -1;
		}
		const bool segmented = g.Mb > 0 && g.Mb < g.M;
		if( ( (size_t)a.W8 % 16 ) != 0 || ( !g.lnX && ( ( (size_t)g.A % 16 ) != 0 || ( g.lda % 8 ) != 0 || g.lda < g.K || ( segmented && ( g.aBatchStride % 8 ) != 0 ) ) ) ||
			( g.lnX && ( ( (size_t)g.lnX | (size_t)g.lnW | (size_t)g.lnB ) % 16 ) != 0 ) )
		{
			setError( "gemvW8: the weight rows, the activation rows and the LayerNorm operands must be 16-byte aligned, the rows at least K apart" );
			return -1;
		}
		// the vector epilogues: four consecutive columns of one activation row as one 16-byte (FP32) or 8-byte (FP16) access
		const bool cols4 = ( g.N % 4 ) == 0 && ( g.ldc % 4 ) == 0 && !segmented && ( (size_t)g.bias % 16 ) == 0;
		a.vecEpi = 0;
		switch( g.epi )
		{
		case EPI_F32:
			if( !g.out32 ) break;
			a.vecEpi = cols4 && ( ( (size_t)g.out32 | (size_t)g.res ) % 16 ) == 0;
			return launchW8E<EPI_F32>( a, stream );
		case EPI_F16_GELU:
			if( !g.out16 || !g.bias ) break;
			a.vecEpi = cols4 && ( (size_t)g.out16 % 8 ) == 0;
			return launchW8E<EPI_F16_GELU>( a, stream );
		case EPI_QKV_DEC:
			if( !g.q || !g.k || !g.v || !g.bias || g.H < 1 || g.N != 3 * g.H * HEAD_DIM || g.nTok < 1 ) break;
			return launchW8E<EPI_QKV_DEC>( a, stream );
		}
		setError( "gemvW8: epilogue EPI_F32 (out32), EPI_F16_GELU (out16, bias) or EPI_QKV_DEC (q, k, v, bias, N = 3 * 64 * H) with its operands" );
		return -1;
	}
}
