// What the GEMM families (gemm_tiled.hip, gemm_persistent.hip, gemm_decode.hip) have in common: the global -> LDS loads in their three forms, the raw
// barrier, the bounds-checked tile epilogue that all three tiled kernels take for their edge tiles -- and, host side, the test the launchers of
// the tiled kernels make before they choose the LDS-transposed epilogue.
#pragma once
#include "kernels.h"
#include "epilogue.h"

namespace wh
{
	namespace
	{
		// one 16-byte-per-lane global -> LDS instruction; M0 (the LDS destination base) is saved and restored inside the
		// statement because the compiler does not preserve it around inline assembly (cdna_hip_programming.md section 5.7)
		__device__ __forceinline__ void ldsDma16( const void* src, unsigned ldsByteAddr )
		{
			unsigned keep;
			asm volatile( "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
						  : "=&s"( keep )
						  : "v"( src ), "s"( ldsByteAddr )
						  : "memory" );
		}
		// Two 16-byte-per-lane global -> LDS instructions (2 x 1 KiB, LDS destinations dst and dst + 1024; global addresses
		// base + off0 / base + off1 with a wave-uniform 64-bit base). M0 (the LDS destination) is saved and restored inside the
		// statement: the compiler does not preserve it around inline assembly (cdna_hip_programming.md section 5.7).
		__device__ __forceinline__ void ldsDmaPair( const void* base, unsigned off0, unsigned off1, unsigned dst )
		{
			unsigned keep;
			// s_nop 1 / s_nop 0: wait states between the scalar writes (M0; a base computed just before the statement) and the
			// memory instruction that reads them -- nothing inside an asm string is padded by the compiler
			asm volatile( "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 1\n\tglobal_load_lds_dwordx4 %2, %1\n\t"
						  "s_mov_b32 m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %1\n\ts_mov_b32 m0, %0"
						  : "=&s"( keep )
						  : "s"( base ), "v"( off0 ), "v"( off1 ), "s"( dst ), "s"( dst + 1024u )
						  : "memory" );
		}
		// the same for one instruction (1 KiB at dst)
		__device__ __forceinline__ void ldsDmaOne( const void* base, unsigned off0, unsigned dst )
		{
			unsigned keep;
			asm volatile( "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 1\n\tglobal_load_lds_dwordx4 %2, %1\n\ts_mov_b32 m0, %0"
						  : "=&s"( keep )
						  : "s"( base ), "v"( off0 ), "s"( dst )
						  : "memory" );
		}
#define WH_BAR() asm volatile( "s_barrier" ::: "memory" )

		// Tile epilogue shared by the staging variants: D[row][col], col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).
		// Same arithmetic per element as epilogueOne, organised for the memory system: the row-dependent index math (the
		// divisions by T) is done once per row instead of once per element, and everything the epilogue READS (residual,
		// position embedding, bias) is requested -- with clamped, hence unconditional, addresses -- before the first store, so
		// a wave pays one memory round trip instead of one per element (the residual is updated in place: a load may not be
		// moved above the preceding store by the compiler).
		template<int EPI, class C>
		__device__ __forceinline__ void tileEpilogue( const GemmArgs& a, f32x16 ( &acc )[ C::TI ][ C::TJ ], int tm, int tn, int wm, int wn, int lane )
		{
			constexpr int BM = C::BM, BN = C::BN;
			const int hi = lane >> 5;
			const int d = a.H * HEAD_DIM;
			int nn[ C::TJ ];
			float bias[ C::TJ ];
#pragma unroll
			for( int j = 0; j < C::TJ; j++ )
			{
				nn[ j ] = tn * BN + wn * 32 * C::TJ + j * 32 + ( lane & 31 );
				const int nc = nn[ j ] < a.N ? nn[ j ] : a.N - 1;
				bias[ j ] = a.bias ? a.bias[ nc ] : 0.0f;
			}
#pragma unroll
			for( int i = 0; i < C::TI; i++ )
			{
				const int mBase = tm * BM + wm * 32 * C::TI + i * 32 + 4 * hi;
				if constexpr( EPI == EPI_F32 || EPI == EPI_CONV2 )
				{
					long long ro[ 16 ], po[ 16 ];
#pragma unroll
					for( int r = 0; r < 16; r++ )
					{
						int m = mBase + ( r & 3 ) + 8 * ( r >> 2 );
						m = m < a.M ? m : a.M - 1;
						if constexpr( EPI == EPI_F32 )
							ro[ r ] = rowOffset( m, a.Mb, a.ldc, a.cBatchStride );
						else
						{
							const int b = m / a.Mb;
							ro[ r ] = (long long)m * a.ldc;
							po[ r ] = (long long)( m - b * a.Mb ) * a.N;
						}
					}
					float ex[ C::TJ ][ 16 ];
#pragma unroll
					for( int j = 0; j < C::TJ; j++ )
					{
						const int nc = nn[ j ] < a.N ? nn[ j ] : a.N - 1;
#pragma unroll
						for( int r = 0; r < 16; r++ )
						{
							if constexpr( EPI == EPI_F32 )
								ex[ j ][ r ] = a.res ? a.res[ ro[ r ] + nc ] : 0.0f;
							else
								ex[ j ][ r ] = a.pe[ po[ r ] + nc ];
						}
					}
#pragma unroll
					for( int j = 0; j < C::TJ; j++ )
					{
						if( nn[ j ] >= a.N ) continue;
#pragma unroll
						for( int r = 0; r < 16; r++ )
						{
							const int m = mBase + ( r & 3 ) + 8 * ( r >> 2 );
							if( m >= a.M ) continue;
							if constexpr( EPI == EPI_F32 )
								a.out32[ ro[ r ] + nn[ j ] ] = ( acc[ i ][ j ][ r ] + bias[ j ] ) + ex[ j ][ r ];
							else
								a.out32[ ro[ r ] + nn[ j ] ] = ex[ j ][ r ] + (float)gelu16( acc[ i ][ j ][ r ] + bias[ j ] );
						}
					}
				}
				else if constexpr( EPI == EPI_F16_GELU )
				{
#pragma unroll
					for( int r = 0; r < 16; r++ )
					{
						const int m = mBase + ( r & 3 ) + 8 * ( r >> 2 );
						if( m >= a.M ) continue;
						const long long ro = rowOffset( m, a.Mb, a.ldc, a.cBatchStride );
#pragma unroll
						for( int j = 0; j < C::TJ; j++ )
							if( nn[ j ] < a.N ) a.out16[ ro + nn[ j ] ] = gelu16( acc[ i ][ j ][ r ] + bias[ j ] );
					}
				}
				else if constexpr( EPI == EPI_QKV_ENC || EPI == EPI_CROSS_KV )
				{
					// column-dependent part of the destination, once per j
					int sel[ C::TJ ];
					long long colOff[ C::TJ ];
#pragma unroll
					for( int j = 0; j < C::TJ; j++ )
					{
						const int n = nn[ j ] < a.N ? nn[ j ] : a.N - 1;
						if constexpr( EPI == EPI_QKV_ENC )
						{
							sel[ j ] = n / d;
							const int c = n - sel[ j ] * d;
							colOff[ j ] = (long long)( c >> 6 ) * ( sel[ j ] == 2 ? (long long)HEAD_DIM * a.Tpad : (long long)a.T * HEAD_DIM ) + ( sel[ j ] == 2 ? 0 : ( c & 63 ) );
						}
						else
						{
							const int layer = n / ( 2 * d );
							const int c2 = n - layer * 2 * d;
							sel[ j ] = c2 >= d ? 1 : 0;
							const int c = sel[ j ] ? c2 - d : c2;
							colOff[ j ] = ( (long long)layer * a.B * a.H + ( c >> 6 ) ) * a.T * HEAD_DIM + ( c & 63 );
						}
					}
					const bool packT = ( a.T & 3 ) == 0;
#pragma unroll
					for( int g = 0; g < 4; g++ )
					{
						// rows mBase + 8 g + {0,1,2,3}: 4 consecutive time steps of one sequence when T % 4 == 0
						const int m0 = mBase + 8 * g;
						const int mc = m0 < a.M ? m0 : a.M - 1;
						const int b0 = mc / a.T;
						const int t0 = mc - b0 * a.T;
#pragma unroll
						for( int j = 0; j < C::TJ; j++ )
						{
							if( nn[ j ] >= a.N ) continue;
							if constexpr( EPI == EPI_QKV_ENC )
							{
								if( sel[ j ] == 2 && packT )
								{
									// fragment-major V: the 4 rows are 4 consecutive keys = 4 consecutive halfs of one fragment
									if( m0 < a.M )
									{
										const int c = nn[ j ] - 2 * d;
										f16x4 pk;
#pragma unroll
										for( int e = 0; e < 4; e++ ) pk[ e ] = (f16)( acc[ i ][ j ][ 4 * g + e ] + bias[ j ] );
										*(f16x4*)( a.v + (long long)b0 * a.H * HEAD_DIM * a.Tpad + colOff[ j ] + vFragIndex( t0, c & 63 ) ) = pk;
									}
									continue;
								}
							}
#pragma unroll
							for( int e = 0; e < 4; e++ )
							{
								const int m = m0 + e;
								if( m >= a.M ) continue;
								int b = b0, t = t0 + e;
								if( !packT && t >= a.T )
								{
									b = m / a.T;
									t = m - b * a.T;
								}
								const float v = acc[ i ][ j ][ 4 * g + e ];
								if constexpr( EPI == EPI_QKV_ENC )
								{
									const float x = v + bias[ j ];
									if( sel[ j ] == 0 )
										a.q[ ( (long long)b * a.H * a.T + t ) * HEAD_DIM + colOff[ j ] ] = (f16)x;
									else if( sel[ j ] == 1 )
										a.k[ ( (long long)b * a.H * a.T + t ) * HEAD_DIM + colOff[ j ] ] = (f16)x;
									else
										a.v[ (long long)b * a.H * HEAD_DIM * a.Tpad + colOff[ j ] + vFragIndex( t, ( nn[ j ] - 2 * d ) & 63 ) ] = (f16)x;
								}
								else
								{
									const long long o = ( (long long)b * a.H * a.T + t ) * HEAD_DIM + colOff[ j ];
									if( sel[ j ] )
										a.v[ o ] = (f16)( v + bias[ j ] );
									else
										a.k[ o ] = (f16)( v * a.scale );
								}
							}
						}
					}
				}
				else
				{
#pragma unroll
					for( int j = 0; j < C::TJ; j++ )
					{
						if( nn[ j ] >= a.N ) continue;
#pragma unroll
						for( int r = 0; r < 16; r++ )
						{
							const int m = mBase + ( r & 3 ) + 8 * ( r >> 2 );
							if( m < a.M )
								epilogueOne<EPI>( a, m, nn[ j ], acc[ i ][ j ][ r ] );
						}
					}
				}
			}
		}
	}	// namespace

	// ---- host side ----
	// The LDS-transposed ("wide") epilogue with 16-byte stores needs whole, aligned chunks. withV: the 4-wave kernel sends the V columns of the encoder's
	// Q/K/V product through it as well, which takes T % 4 == 0 and an aligned a.v.
	inline bool wideEpilogueOk( const GemmArgs& a, int epi, bool withV = false )
	{
		if( !( g_tuning & TUNE_GEMM_WIDE_EPI ) ) return false;
		const bool al16 = ( a.N % 8 ) == 0 && ( a.ldc % 8 ) == 0 && ( a.cBatchStride % 8 ) == 0;
		switch( epi )
		{
		case EPI_F32: return al16 && ( ( (size_t)a.out32 | (size_t)a.res ) % 16 ) == 0;
		case EPI_CONV2: return al16 && ( ( (size_t)a.out32 | (size_t)a.pe ) % 16 ) == 0;
		case EPI_F16_GELU: return al16 && ( (size_t)a.out16 % 16 ) == 0;
		case EPI_QKV_ENC: return ( a.N % 64 ) == 0 && ( ( (size_t)a.q | (size_t)a.k ) % 16 ) == 0 && ( !withV || ( ( a.T % 4 ) == 0 && ( (size_t)a.v % 16 ) == 0 ) );
		case EPI_CROSS_KV: return ( a.N % 64 ) == 0 && ( ( (size_t)a.k | (size_t)a.v ) % 16 ) == 0;
		}
		return false;
	}
}
