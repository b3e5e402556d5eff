// NT GEMM for gfx950: FP16 x FP16 -> FP32 on MFMA, fused epilogues. This unit decides which kernel family takes a product.
// Replaces ComputeShaders/mulMatTiled.hlsl (32x32 LDS tiles, FP32 FMA) and mulMatByRowTiled.hlsl (GEMV) of the
// reference, with the numerics of the reference's CPU path: activations are FP16 (rounded by the producer, which is
// what ggml does before every weight product, Whisper/source/ggml.c:4588-4611), weights FP16, accumulation FP32.
// gemm_tiled.hip       gemmTiled: a workgroup per output tile, 128x128x32 or 256x256x64 -- any product, any epilogue
// gemm_persistent.hip  gemmTiled8 / gemmTiled4: one workgroup per CU walks 256x256x64 tiles -- the encoder's products several clips deep
// gemm_decode.hip      gemmSkinny, gemvFused, gemmAllRows, gemmDecRows, gemmDecTile: the decode step's few rows (launchGemmSkinny, launchGemv)
// gemm_device.h        the device helpers they share; gemm_launch.h: what the units call of each other
#include "gemm_launch.h"
#include <stdlib.h>

namespace wh
{
	int checkGemmArgs( const GemmArgs& a )
	{
		if( a.M <= 0 || a.N <= 0 || a.K <= 0 || ( a.K % 64 ) != 0 )
		{
			setError( "gemm: M, N must be positive and K a positive multiple of 64" );
			return -1;
		}
		if( ( a.lda % 8 ) != 0 || ( a.aBatchStride % 8 ) != 0 )
		{
			setError( "gemm: A rows must be 16-byte aligned" );
			return -1;
		}
		return 0;
	}

	thread_local int t_gemmWideEpi = 0;

	eGemmFamily chooseGemmFamily( const GemmArgs& a )
	{
		// big tiles only when they still give every CU a workgroup and M is several clips deep
		const bool big = (long long)( ( a.M + 255 ) / 256 ) * ( ( a.N + 255 ) / 256 ) >= 300 && a.M >= g_opt.gemmBigMinRows && ( g_tuning & TUNE_GEMM_BIG );
		// gemmTiled8 addresses its operands as a 64-bit base + 32-bit byte offsets
		const long long aBytes = 2ll * ( a.Mb > 0 && a.Mb < a.M ? ( (long long)( a.M / a.Mb ) + 1 ) * a.aBatchStride + (long long)a.Mb * a.lda : (long long)a.M * a.lda ) + 2ll * a.K;
		const bool fits32 = aBytes < ( 1ll << 32 ) && 2ll * a.N * a.K < ( 1ll << 32 );
		const bool w8 = big && fits32 && ( g_tuning & TUNE_GEMM_8WAVE ) != 0 && persistentEpilogue( a.epi );
		// gemmTiled4 on top: at least two K tiles, A segments of at least a tile's 256 rows with a non-negative gap
		// WH_GEMM_4WAVE_EPIS: bit mask of epilogues that take gemmTiled4 without the tuning bit (A/B runs)
		static const int epis4 = []() { const char* e = getenv( "WH_GEMM_4WAVE_EPIS" ); return e ? atoi( e ) : 0; }();
		const bool w4 = w8 && a.K >= 256 && ( ( g_tuning & TUNE_GEMM_4WAVE ) != 0 || ( ( epis4 >> a.epi ) & 1 ) != 0 ) &&	   // (K >= 256: the FP16 epilogues leave under the next tile's first four K tiles)
			( a.Mb <= 0 || a.Mb >= a.M || ( a.Mb >= 256 && a.aBatchStride >= (long long)a.Mb * a.lda ) );
		if( w4 ) return GEMM_TILED4;
		if( w8 ) return GEMM_TILED8;
		return big && tiledBigEpilogue( a.epi ) ? GEMM_TILED_256 : GEMM_TILED_128;	   // (gemmTiled ignores `big` for the epilogues it has no 256-wide instance of)
	}

	int launchGemm( const GemmArgs& a, hipStream_t stream )
	{
		WH_CHECK( checkGemmArgs( a ) );
		switch( chooseGemmFamily( a ) )
		{
		case GEMM_TILED4: return launchTiled4( a, stream );
		case GEMM_TILED8: return launchTiled8( a, g_opt.gemmMf16 == 1, stream );
		case GEMM_TILED_256: return launchTiled( a, true, stream );
		case GEMM_TILED_128: break;
		}
		return launchTiled( a, false, stream );
	}

	// Tile-shape experiments on the plain FP32 epilogue (tools/gemm_probe.py): the persistent kernels here, gemmTiled's configurations in its unit
	int launchGemmVariant( const GemmArgs& a, int variant, hipStream_t stream )
	{
		switch( variant )
		{
		case 40: return launchTiled8( a, false, stream );	   // the 8-wave persistent kernel (round 3)
		case 52: return launchTiled8( a, true, stream );	   // the same with v_mfma_f32_16x16x32_f16 in the K loop (round 6)
		case 50: return launchTiled4( a, stream );	   // the 4-wave persistent kernel (round 4)
#ifdef WH_PROBES
		case 51: return launchTiled4Probe( a, stream );	   // correct: without the early W pieces / the counted wait after the epilogue
#endif
		}
		return launchTiledVariant( a, variant, stream );
	}
}
