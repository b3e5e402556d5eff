// gemmI8: the NT product of the INT8 encoder path, int8 x int8 -> int32 on the matrix cores, then the row and column scales and the FP16 path's epilogues.
//   acc[m][n] = sum_k qa[m][k] * qw[n][k]                     exact in int32 (|acc| <= 127^2 K)
//   y         = ( (float)acc * sa[m] ) * sw[n]                int32 -> FP32 to nearest even, two multiplications that round separately
//   then epilogueOne's arithmetic (epilogue.h) on y in place of the FP32 accumulator: EPI_F32, EPI_F16_GELU, EPI_QKV_ENC.
// The unit is built with -ffp-contract=off (build.py): y + bias must not become a fused multiply-add of the second scale.
//
// Design (DESIGN.md section 7 "INT8 encoder products" has the measurements)
//   * Tiles and CUs. A workgroup of 4 waves per 128 x 128 output tile, 65 KiB of LDS, 127 .. 138 VGPRs on the row-store path: TWO workgroups live on a CU. That is the answer to
//     the epilogue's share: an int8 tile has half the K tiles of an FP16 one, so a persistent workgroup that owns its CU (gemm_persistent.hip) would spend
//     twice the share of its time storing with the matrix cores idle; here one workgroup's epilogue runs under the other's K loop, and nothing has to be
//     scheduled by hand. Block ids are remapped so that every XCD (id % 8) walks a contiguous range of tiles, in bands of 8 M tiles column by column: the
//     band's A rows (8 x 128 x K bytes) stay in that XCD's L2 while each W tile is fetched once per band.
//   * LDS image. BK = 128: a tile row is one 128-byte line of 128 int8, 8 chunks of 16 bytes. Tiles go global -> LDS directly (global_load_lds_dwordx4: a wave
//     instruction lays down 8 whole rows), the chunk index XORed with ( row >> 1 ) & 7 on the SOURCE side and again when fragments are read, which makes the
//     16-byte fragment reads of 32 rows conflict free. Byte for byte the image of gemmTiled's 256 x 256 x 64 FP16 configuration; the K loop has half the steps.
//   * MFMA form. v_mfma_i32_32x32x32_i8: 16 bytes per lane and operand (lane l: row l & 31, bytes 16 ( l >> 5 ) .. + 15 of the 32-byte k-substep), a wave
//     owns 64 x 64 = 2 x 2 of them, so a k-substep reads 4 fragments for 4 instructions. The 16x16x64 form would read 8 fragments for 16 instructions of a
//     quarter the work each -- twice the LDS bytes per multiply-add -- and the 32x32 accumulator layout (a lane holds one column, rows ( r & 3 ) + 8 ( r >> 2 )
//     + 4 ( l >> 5 )) is the one the shared bounds-checked epilogue (gemm_device.h tileEpilogue) is written for. Which k a byte of a fragment stands for does
//     not matter as long as A and W agree: the sum is an integer sum.
//   * Prefetch. Two LDS stages: tile kt + 1 is requested right behind the barrier that opens step kt and lands while tile kt is multiplied; with the
//     neighbour workgroup's stages that is four tiles in flight per CU.
//   * Scales. sa of the tile's 128 rows and sw of its 128 columns are requested by one load per thread BEFORE the first K tile is awaited and parked in 1 KiB
//     of LDS behind the stages when the first tile has landed; the epilogue reads them from LDS, never from memory.
//   * Epilogue. The wave's raw int32 block goes through the (now idle) stage memory, 32 rows at a time, XOR-swizzled, and is read back along rows: a lane
//     then owns 4 (FP32 outputs) or 8 (FP16 outputs) consecutive columns of one row, converts, scales, adds bias / residual or applies GELU, and leaves
//     16-byte row stores; what it reads from memory (bias, residual) is requested before the first store. The V columns of the Q/K/V product (fragment-major,
//     8-byte stores of 4 keys) and any product whose buffers are not 16-byte aligned take tileEpilogue with y in the accumulator's place. Edge tiles in M:
//     loads clamped to the last row, stores masked.
// Serves any M, N % 128 == 0, K % 128 == 0.
#include "gemm_device.h"
#include "gemm_launch.h"

namespace wh
{
	namespace
	{
		typedef __attribute__( ( ext_vector_type( 4 ) ) ) int i32x4;
		typedef __attribute__( ( ext_vector_type( 16 ) ) ) int i32x16;

		struct CfgI8
		{
			static constexpr int BM = 128, BN = 128, BK = 128, TI = 2, TJ = 2, NT = 256, NBUF = 2;
			static constexpr int A_BYTES = BM * BK, STAGE = ( BM + BN ) * BK;
			static constexpr int SCALES_AT = NBUF * STAGE, LDS_BYTES = SCALES_AT + ( BM + BN ) * 4;
			static constexpr int GROUP_M = 8;
		};
		static_assert( CfgI8::NT / 64 * 8192 <= CfgI8::SCALES_AT, "the epilogue's staging lies inside the operand stages" );

		// byte position of logical 16-byte chunk c of tile row `row`
		__device__ __forceinline__ int i8Offset( int row, int c ) { return row * CfgI8::BK + ( ( c ^ ( ( row >> 1 ) & 7 ) ) << 4 ); }

		__device__ __forceinline__ void waveSync()
		{
			__builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront" );
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront" );
		}

		// gelu16 (common.h) with its last step pinned. fp16( f * rcp ) is ONE v_fma_mixlo_f16 there -- a single rounding of the exact product -- wherever hipcc
		// converts element by element, which is the case in the kernels the op-level tests take gelu16's table from. In the 8-wide row code below it would
		// select v_pk_mul_f32 + v_cvt_pk_f16_f32 instead: two roundings, one FP16 ulp apart on 2e-4 of the arguments. The arithmetic in front of it is gelu16's.
		__device__ __forceinline__ f16 gelu16Pinned( float x )
		{
			const float f = round16( x );
			constexpr float C1 = -2.0f * 0.79788456080286535587989211986876f * 1.44269504088896340736f;
			constexpr float C2 = C1 * 0.044715f;
			const float e = __builtin_amdgcn_exp2f( fmaf( f * f, C2, C1 ) * f );
			const float r = __builtin_amdgcn_rcpf( 1.0f + e );
			unsigned lo;
			asm( "v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"( lo ) : "v"( f ), "v"( r ) );
			return __builtin_bit_cast( f16, (unsigned short)lo );
		}

		template<int EPI, bool WIDE>
		__global__ void __launch_bounds__( CfgI8::NT, 2 ) gemmI8( const GemmI8Args p )
		{
			using C = CfgI8;
			constexpr int BM = C::BM, BN = C::BN, BK = C::BK;
			const GemmArgs& a = p.g;
			extern __shared__ __attribute__( ( aligned( 16 ) ) ) unsigned char smem[];
			float* const ldsScale = (float*)( smem + C::SCALES_AT );	  // [0, 128) sa of the tile's rows, [128, 256) sw of its columns

			const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
			const int wm = wave >> 1, wn = wave & 1;
			const int tilesN = a.N / BN, tilesM = ( a.M + BM - 1 ) / BM;
			int lin;
			{
				const int nb = gridDim.x, bid = blockIdx.x;
				const int q = nb >> 3, r = nb & 7;
				const int xcd = bid & 7, idx = bid >> 3;
				lin = ( xcd < r ? xcd * ( q + 1 ) : r * ( q + 1 ) + ( xcd - r ) * q ) + idx;
			}
			int tm, tn;
			{
				const int perBand = C::GROUP_M * tilesN;
				const int band = lin / perBand;
				const int first = band * C::GROUP_M;
				const int rows = min( tilesM - first, C::GROUP_M );
				const int r = lin - band * perBand;
				tm = first + r % rows;
				tn = r / rows;
			}

			// this thread's scale: threads 0 .. 127 the rows' (clamped at the edge), 128 .. 255 the columns'
			const float* scaleSrc;
			{
				const int t = tid & 127;
				int m = tm * BM + t;
				m = m < a.M ? m : a.M - 1;
				scaleSrc = tid < 128 ? p.sa + m : p.sw + tn * BN + t;
			}

			const int rIn = lane >> 3, cPhys = lane & 7;
			const int8_t* gA[ 4 ];
			const int8_t* gW[ 4 ];
#pragma unroll
			for( int i = 0; i < 4; i++ )
			{
				const int row = ( wave * 4 + i ) * 8 + rIn;
				const int c = cPhys ^ ( ( row >> 1 ) & 7 );
				int m = tm * BM + row;
				m = m < a.M ? m : a.M - 1;
				gA[ i ] = p.A8 + (long long)m * a.lda + c * 16;
				gW[ i ] = p.W8 + (long long)( tn * BN + row ) * a.K + c * 16;
			}
			typedef __attribute__( ( address_space( 3 ) ) ) void* LdsPtr;
			typedef const __attribute__( ( address_space( 1 ) ) ) void* GlobalPtr;
			auto issue = [ & ]( int kt, int buf )
			{
				unsigned char* const dstA = smem + buf * C::STAGE + wave * 4096;
				unsigned char* const dstW = dstA + C::A_BYTES;
				const int ko = kt * BK;
#pragma unroll
				for( int i = 0; i < 4; i++ )
					__builtin_amdgcn_global_load_lds( (GlobalPtr)( gA[ i ] + ko ), (LdsPtr)( dstA + i * 1024 ), 16, 0, 0 );
#pragma unroll
				for( int i = 0; i < 4; i++ )
					__builtin_amdgcn_global_load_lds( (GlobalPtr)( gW[ i ] + ko ), (LdsPtr)( dstW + i * 1024 ), 16, 0, 0 );
			};

			i32x16 acc[ 2 ][ 2 ];
#pragma unroll
			for( int i = 0; i < 2; i++ )
#pragma unroll
				for( int j = 0; j < 2; j++ )
#pragma unroll
					for( int r = 0; r < 16; r++ ) acc[ i ][ j ][ r ] = 0;

			const int nk = a.K / BK;
			const int fragRow = lane & 31, fragC = lane >> 5;
			issue( 0, 0 );
			const float scaleV = *scaleSrc;
			for( int kt = 0; kt < nk; kt++ )
			{
				const int buf = kt & 1;
				asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
				__syncthreads();
				if( kt == 0 ) ldsScale[ tid ] = scaleV;	   // visible behind the next barrier: the next step's, or the one in front of the epilogue
				if( kt + 1 < nk ) issue( kt + 1, buf ^ 1 );
				const unsigned char* const ldsA = smem + buf * C::STAGE;
				const unsigned char* const ldsW = ldsA + C::A_BYTES;
#pragma unroll
				for( int ks = 0; ks < BK / 32; ks++ )
				{
					i32x4 fa[ 2 ], fb[ 2 ];
#pragma unroll
					for( int i = 0; i < 2; i++ )
					{
						fa[ i ] = *(const i32x4*)( ldsA + i8Offset( wm * 64 + i * 32 + fragRow, ks * 2 + fragC ) );
						fb[ i ] = *(const i32x4*)( ldsW + i8Offset( wn * 64 + i * 32 + fragRow, ks * 2 + fragC ) );
					}
#pragma unroll
					for( int i = 0; i < 2; i++ )
#pragma unroll
						for( int j = 0; j < 2; j++ )
							acc[ i ][ j ] = __builtin_amdgcn_mfma_i32_32x32x32_i8( fa[ i ], fb[ j ], acc[ i ][ j ], 0, 0, 0 );
				}
			}
			__syncthreads();	// every wave is done with the stages; the scales are in LDS

			const float* const sa = ldsScale + wm * 64;
			const float* const sw = ldsScale + 128 + wn * 64;
			const int hi = lane >> 5, c = lane & 31;
			const int m0 = tm * BM + wm * 64, n0 = tn * BN + wn * 64;
			const int d = a.H * HEAD_DIM;
			const bool vPart = EPI == EPI_QKV_ENC && n0 >= 2 * d;	   // wave-uniform: a wave's 64 columns are one head
			if( !WIDE || vPart )
			{
				f32x16 y[ 2 ][ 2 ];
#pragma unroll
				for( int i = 0; i < 2; i++ )
#pragma unroll
					for( int j = 0; j < 2; j++ )
#pragma unroll
						for( int r = 0; r < 16; r++ )
							y[ i ][ j ][ r ] = ( (float)acc[ i ][ j ][ r ] * sa[ i * 32 + ( r & 3 ) + 8 * ( r >> 2 ) + 4 * hi ] ) * sw[ j * 32 + c ];
				tileEpilogue<EPI, C>( a, y, tm, tn, wm, wn, lane );
				return;
			}

			int* const L = (int*)( smem + wave * 8192 );	   // [32 rows][64 columns] int32, 16-byte chunk index ^ ( row & 15 )
			auto stageHalf = [ & ]( int i )
			{
#pragma unroll
				for( int j = 0; j < 2; j++ )
#pragma unroll
					for( int r = 0; r < 16; r++ )
					{
						const int row = ( r & 3 ) + 8 * ( r >> 2 ) + 4 * hi;
						const int col = j * 32 + c;
						L[ row * 64 + ( ( ( col >> 2 ) ^ ( row & 15 ) ) << 2 ) + ( col & 3 ) ] = acc[ i ][ j ][ r ];
					}
			};
			if constexpr( EPI == EPI_F32 )
			{
				const int chunk = lane & 15;
				const int n = n0 + chunk * 4;
				const f32x4 sw4 = *(const f32x4*)( sw + chunk * 4 );
				const f32x4 bias = a.bias ? *(const f32x4*)( a.bias + n ) : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
				for( int i = 0; i < 2; i++ )
				{
					if( i == 1 ) waveSync();
					stageHalf( i );
					waveSync();
#pragma unroll
					for( int g4 = 0; g4 < 2; g4++ )
					{
						f32x4 ex[ 4 ];
						long long off[ 4 ];
#pragma unroll
						for( int u = 0; u < 4; u++ )
						{
							int m = m0 + i * 32 + ( g4 * 4 + u ) * 4 + ( lane >> 4 );
							m = m < a.M ? m : a.M - 1;
							off[ u ] = rowOffset( m, a.Mb, a.ldc, a.cBatchStride ) + n;
							ex[ u ] = a.res ? *(const f32x4*)( a.res + off[ u ] ) : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
						}
#pragma unroll
						for( int u = 0; u < 4; u++ )
						{
							const int row = ( g4 * 4 + u ) * 4 + ( lane >> 4 );
							if( m0 + i * 32 + row >= a.M ) continue;
							const i32x4 v = *(const i32x4*)( L + row * 64 + ( ( chunk ^ ( row & 15 ) ) << 2 ) );
							const float sr = sa[ i * 32 + row ];
							f32x4 o;
#pragma unroll
							for( int e = 0; e < 4; e++ ) o[ e ] = ( ( ( (float)v[ e ] * sr ) * sw4[ e ] ) + bias[ e ] ) + ex[ u ][ e ];
							*(f32x4*)( a.out32 + off[ u ] ) = o;
						}
					}
				}
			}
			else
			{
				// FP16 outputs: 8 columns of a row per lane
				const int chunk = lane & 7;
				const int n = n0 + chunk * 8;
				f32x4 sw8[ 2 ], bias[ 2 ];
#pragma unroll
				for( int h = 0; h < 2; h++ )
				{
					sw8[ h ] = *(const f32x4*)( sw + chunk * 8 + h * 4 );
					bias[ h ] = *(const f32x4*)( a.bias + n + h * 4 );
				}
				int sel = 0, head = 0;
				if constexpr( EPI == EPI_QKV_ENC )
				{
					sel = n0 / d;
					head = ( n0 - sel * d ) >> 6;
				}
#pragma unroll
				for( int i = 0; i < 2; i++ )
				{
					if( i == 1 ) waveSync();
					stageHalf( i );
					waveSync();
#pragma unroll
					for( int it = 0; it < 4; it++ )
					{
						const int row = it * 8 + ( lane >> 3 );
						const int m = m0 + i * 32 + row;
						if( m >= a.M ) continue;
						const float sr = sa[ i * 32 + row ];
						f16x8 hv;
#pragma unroll
						for( int h = 0; h < 2; h++ )
						{
							const i32x4 v = *(const i32x4*)( L + row * 64 + ( ( ( chunk * 2 + h ) ^ ( row & 15 ) ) << 2 ) );
#pragma unroll
							for( int e = 0; e < 4; e++ )
							{
								const float x = ( ( (float)v[ e ] * sr ) * sw8[ h ][ e ] ) + bias[ h ][ e ];
								hv[ h * 4 + e ] = EPI == EPI_F16_GELU ? gelu16Pinned( x ) : (f16)x;
							}
						}
						if constexpr( EPI == EPI_F16_GELU )
							*(f16x8*)( a.out16 + rowOffset( m, a.Mb, a.ldc, a.cBatchStride ) + n ) = hv;
						else
						{
							const int b = m / a.T;
							const int t = m - b * a.T;
							f16* const dst = sel == 0 ? a.q : a.k;
							*(f16x8*)( dst + ( ( (long long)b * a.H + head ) * a.T + t ) * HEAD_DIM + chunk * 8 ) = hv;
						}
					}
				}
			}
		}

		template<int EPI>
		int launchGemmI8E( const GemmI8Args& p, bool wide, hipStream_t stream )
		{
			const GemmArgs& a = p.g;
			const dim3 grid( ( a.M + CfgI8::BM - 1 ) / CfgI8::BM * ( a.N / CfgI8::BN ) );
			t_gemmWideEpi = wide ? 1 : 0;
			if( wide ) return launchLds<gemmI8<EPI, true>>( grid, dim3( CfgI8::NT ), CfgI8::LDS_BYTES, stream, p );
			return launchLds<gemmI8<EPI, false>>( grid, dim3( CfgI8::NT ), CfgI8::LDS_BYTES, stream, p );
		}
	}	// namespace

	int launchGemmI8( const GemmI8Args& p, hipStream_t stream )
	{
		const GemmArgs& a = p.g;
		if( !p.A8 || !p.W8 || !p.sa || !p.sw || a.M <= 0 || a.N <= 0 || ( a.N % 128 ) != 0 || a.K <= 0 || ( a.K % 128 ) != 0 || a.K > 65536 || a.lda < a.K || ( a.lda % 16 ) != 0 ||
			( ( (size_t)p.A8 | (size_t)p.W8 ) % 16 ) != 0 || (long long)( ( a.M + 127 ) / 128 ) * ( a.N / 128 ) > 0x7fffffffll )
		{
			setError( "gemmI8: N and K must be multiples of 128 (K at most 65536), the int8 operands 16-byte aligned with rows at least K apart, both scale arrays given" );
			return -1;
		}
		const bool al = ( ( a.ldc | a.cBatchStride ) % 8 ) == 0 && ( (size_t)a.bias % 16 ) == 0;
		switch( a.epi )
		{
		case EPI_F32:
			if( !a.out32 ) break;
			return launchGemmI8E<EPI_F32>( p, al && ( ( (size_t)a.out32 | (size_t)a.res ) % 16 ) == 0, stream );
		case EPI_F16_GELU:
			if( !a.out16 || !a.bias ) break;
			return launchGemmI8E<EPI_F16_GELU>( p, al && ( (size_t)a.out16 % 16 ) == 0, stream );
		case EPI_QKV_ENC:
			if( !a.q || !a.k || !a.v || !a.bias || a.H <= 0 || a.N != 3 * a.H * HEAD_DIM || a.T <= 0 || ( a.M % a.T ) != 0 ) break;
			return launchGemmI8E<EPI_QKV_ENC>( p, ( (size_t)a.bias % 16 ) == 0 && ( ( (size_t)a.q | (size_t)a.k ) % 16 ) == 0, stream );
		default:
			setError( "gemmI8: the epilogues of the INT8 path are EPI_F32, EPI_F16_GELU and EPI_QKV_ENC" );
			return -1;
		}
		setError( "gemmI8: an operand of the epilogue is null or does not fit its shape" );
		return -1;
	}
}
