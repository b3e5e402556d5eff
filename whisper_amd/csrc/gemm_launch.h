// What the GEMM units ask of each other. gemm.hip decides which family takes a product; a family picks its kernel instance from a.epi in its own
// unit. The public entry points (launchGemm, launchGemmSkinny, launchGemv, launchGemmVariant) are declared in kernels.h.
#pragma once
#include "kernels.h"

namespace wh
{
	// gemm.hip
	int checkGemmArgs( const GemmArgs& a );
	// which family launchGemm gives a product to, under the tuning bits and options of the moment (the values are wh_gemm_family's, include/whisper_hip.h)
	enum eGemmFamily : int
	{
		GEMM_TILED_128 = 0,	 // gemmTiled, 128x128x32 tiles
		GEMM_TILED_256 = 1,	 // gemmTiled, 256x256x64 tiles
		GEMM_TILED8 = 2,	 // gemmTiled8
		GEMM_TILED4 = 3,	 // gemmTiled4
	};
	eGemmFamily chooseGemmFamily( const GemmArgs& a );
	// the GemmArgs::wideEpi of the calling thread's last launch of a tiled family: 0 = column stores, 1 = the LDS-transposed epilogue, 2 = that with the lean
	// epilogue on interior tiles. Written by the families' launchers for wh_op_gemm_encoder to report; nothing reads it to decide anything.
	extern thread_local int t_gemmWideEpi;

	// gemm_tiled.hip -- gemmTiled, a workgroup per output tile: 256x256x64 tiles with big, else 128x128x32; any epilogue
	int launchTiled( const GemmArgs& a, bool big, hipStream_t stream );
	bool tiledBigEpilogue( int epi );	 // false: the epilogue is built with the 128x128x32 tiles only, `big` changes nothing (EPI_CONV2, the decoder's)
	// the tile-shape variants of launchGemmVariant that are gemmTiled configurations (EPI_F32)
	int launchTiledVariant( const GemmArgs& a, int variant, hipStream_t stream );

	// gemm_persistent.hip -- 256x256x64 tiles walked by one workgroup per CU, the epilogues of persistentEpilogue() only. The caller has checked
	// what the kernels assume about the operands (launchGemm: 32-bit offsets; for the 4-wave kernel K and the A segments as well).
	bool persistentEpilogue( int epi );
	int launchTiled8( const GemmArgs& a, bool mf16, hipStream_t stream );	 // gemmTiled8; mf16: the K loop on v_mfma_f32_16x16x32_f16 (option gemm_mf16)
	int launchTiled4( const GemmArgs& a, hipStream_t stream );				 // gemmTiled4
#ifdef WH_PROBES
	int launchTiled4Probe( const GemmArgs& a, hipStream_t stream );			 // EPI_F32 without the early W pieces / the counted wait after the epilogue
#endif
}
