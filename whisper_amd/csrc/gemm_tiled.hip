// gemmTiled: the NT GEMM with a workgroup per output tile (FP16 x FP16 -> FP32 on v_mfma_f32_32x32x16_f16, fused epilogues).
//
// gemmTiled<EPI, TileCfg>: every wave owns a 64x64 output sub-tile (2x2 MFMA tiles); a workgroup is 128x128x32 (4 waves,
//   3 workgroups per CU) or, for GEMMs several clips deep, 256x256x64 (16 waves). Tiles go global -> LDS directly
//   (global_load_lds_dwordx4, double buffered, one barrier per K step): the LDS image of such a load is lane-linear, so
//   rows are unpadded and the conflict-free placement is an XOR of the 16-byte chunk index with the row, applied to the
//   per-lane SOURCE address and again when the 32x32x16 fragments are read (lane l reads row l&31, chunk (l>>5)). The
//   register-staged pipeline with padded rows (144 B / 80 B, conflict free as well) is kept as the A/B alternative.
//   Block ids are remapped so that each XCD (block id % 8) owns a contiguous band of M tiles: the band's A rows are
//   fetched from HBM once per XCD and stay in that XCD's 4 MiB L2 while the (small) weight matrix is re-read from L2.
//   The epilogue requests everything it reads before its first store and does the per-row index math once per row.
#include "gemm_device.h"
#include "gemm_launch.h"

namespace wh
{
	namespace
	{

		// Tile configuration: every wave owns a 64x64 sub-tile (2x2 MFMA 32x32x16 tiles), waves are laid out WAVES_M x WAVES_N.
		// MINW = waves per SIMD the register allocator must leave room for (blocks per CU * waves per block / 4).
		// GL = tiles go global -> LDS directly (global_load_lds_dwordx4, no staging registers): the LDS image of a wave's
		// instruction is lane-linear (base + lane * 16 bytes), so rows are unpadded and the bank-conflict-free placement is
		// an XOR of the 16-byte chunk index applied to the SOURCE address and again when the fragments are read.
		// A wave owns TI x TJ MFMA tiles of 32x32 (default 2 x 2 = 64x64); 4 x 2 reads 6 fragments for 8 MFMAs instead of 4 for 4,
		// which is what the LDS bandwidth of a CU asks for.
		// NBUF (GL only) = LDS stages: 2 = the next tile lands while this one is multiplied (wait for everything at the top of
		// a K step); 3 or 4 = one or two MORE tiles stay in flight across the step's barrier (counted vmcnt + raw s_barrier),
		// which is what covers an HBM round trip that is longer than one K step.
		// PIPE: see below (fragment prefetch / loads spread behind the MFMA groups).
		template<int BM_, int BN_, int BK_, int MINW_, int PF_, bool GL_ = false, int TI_ = 2, int TJ_ = 2, int NBUF_ = 2, int PIPE_ = 0>
		struct TileCfg
		{
			static constexpr int BM = BM_, BN = BN_, BK = BK_, MINW = MINW_, PF = PF_, TI = TI_, TJ = TJ_, NBUF = NBUF_;
			// PIPE (GL only): 1 = FRAGPF, the MFMA fragments of k-substep s+1 are read from LDS before the MFMAs of substep s are
			// issued (two register sets; hipcc on its own re-uses one set, so every substep starts with an exposed LDS round trip).
			// (Issuing the next tile's direct-to-LDS loads one or two at a time behind the MFMA groups instead of as a burst at the
			// top of the K step was measured too: no difference, profiles/r02_gemm_kloop_ablation.txt.)
			static constexpr bool FRAGPF = PIPE_ >= 1;
			static constexpr bool GL = GL_;
			static constexpr int WAVES_M = BM / ( 32 * TI ), WAVES_N = BN / ( 32 * TJ ), NT = WAVES_M * WAVES_N * 64;
			static_assert( GL || ( TI == 2 && TJ == 2 ), "the register-staged path is written for 64x64 wave tiles" );
			static constexpr int STRIDE = GL ? BK : BK + 8;		 // halfs per LDS row: padded 144 B (BK 64) / 80 B (BK 32) are conflict free
			static constexpr int RPI = 512 / BK;				 // GL: tile rows one wave instruction covers (1 KB)
			static constexpr int RPB = 128 / BK;				 // GL: tile rows per 256-byte bank row
			static constexpr int IA = BM / RPI / ( NT / 64 ), IW = BN / RPI / ( NT / 64 );	 // GL: instructions per wave and tile
			static constexpr int A_HALFS = BM * STRIDE, W_HALFS = BN * STRIDE, STAGE = A_HALFS + W_HALFS;
			// the LDS-transposed epilogue (tileEpilogueWide) takes 8 KiB per wave once the operand tiles are dead
			static constexpr int LDS_BYTES = ( NBUF * STAGE * 2 > ( GL ? NT / 64 * 8192 : 0 ) ) ? NBUF * STAGE * 2 : NT / 64 * 8192;
			static_assert( NBUF == 2 || GL, "more than two stages only with direct-to-LDS staging" );
			static constexpr int CPR = BK / 8;					 // 16-byte chunks per tile row
			static constexpr int CA = BM * CPR / NT, CW = BN * CPR / NT;
			static_assert( CA >= 1 && CW >= 1 && BM * CPR % NT == 0 && BN * CPR % NT == 0, "tile does not divide over the threads" );
		};
		// Measured on MI355X (tools/gemm_probe.py, profiles/r01_gemm_tile_probe.txt), M = 10500: 256x256x64 wins when the grid
		// still fills the chip (N >= 2048: 593-662 TFLOP/s), 128x128x32 (3 blocks per CU) wins on narrow outputs and small M;
		// the two-tile-deep prefetch (PF = 2) measured 3-5 % slower than PF = 1 at every shape.
		using CfgDefault = TileCfg<128, 128, 32, 3, 1>;
		using CfgBig = TileCfg<256, 256, 64, 4, 1>;
		using CfgGl = TileCfg<128, 128, 32, 3, 1, true>;
		using CfgGlBig = TileCfg<256, 256, 64, 4, 1, true>;
		using CfgGlPf = TileCfg<128, 128, 32, 3, 1, true, 2, 2, 2, 1>;
		using CfgGlBigPf = TileCfg<256, 256, 64, 4, 1, true, 2, 2, 2, 1>;

		// physical position (in halfs) of logical 16-byte chunk c of tile row `row` in a GL tile
		template<class C>
		__device__ __forceinline__ int glOffset( int row, int c )
		{
			return row * C::BK + ( ( c ^ ( ( row / C::RPB ) % C::CPR ) ) << 3 );
		}

		// ---------------------------------------------------------------------------------------------------------------
		// Wide epilogue: the wave's 64x64 accumulator block goes through the (now idle) LDS tile memory and leaves as 16-byte
		// stores along the rows of the destination. In the MFMA accumulator layout a lane holds ONE column and 16 rows of
		// each 32x32 tile, so a direct epilogue issues 64 two- or four-byte stores per lane (and as many residual loads);
		// per 256x256 tile that is 1024 wave-level store instructions of 64-128 useful bytes, and the tile's fixed cost
		// (24 us against 28 us of K loop at K = 1024, profiles/r01_gemm_tile_probe.txt) was mostly their issue time.
		// Through LDS a lane stores 8 x 16 bytes (FP16 outputs) or loads + stores 16 x 16 bytes (FP32 outputs with residual).
		// LDS image per wave: [64 rows][64 cols] FP16 (8 KiB) or [32 rows][64 cols] FP32 (8 KiB, two halves), 16-byte chunk
		// index XORed with the row so that both the column-wise writes and the row-wise reads are conflict free.
		// Same arithmetic per element as the direct epilogue. Preconditions (checked by the launcher, a.wideEpi): N % 8 == 0,
		// 16-byte aligned rows, T % 8 == 0 irrelevant (rows are independent), a wave's 64 columns inside one head.
		template<int EPI, class C>
		__device__ __forceinline__ void tileEpilogueWide( const GemmArgs& a, f32x16 ( &acc )[ C::TI ][ C::TJ ], int tm, int tn, int wm, int wn, int lane,
			unsigned char* ldsWave )
		{
			static_assert( C::TI == 2 && C::TJ == 2, "64x64 wave tiles" );
			constexpr int BM = C::BM, BN = C::BN;
			const int hi = lane >> 5, c = lane & 31;
			const int d = a.H * HEAD_DIM;
			const int m0 = tm * BM + wm * 64, n0 = tn * BN + wn * 64;
			float bias[ 2 ];
	#pragma unroll
			for( int j = 0; j < 2; j++ )
			{
				const int n = n0 + j * 32 + c;
				bias[ j ] = ( a.bias && n < a.N ) ? a.bias[ n ] : 0.0f;
			}
			if constexpr( EPI == EPI_F16_GELU || EPI == EPI_QKV_ENC || EPI == EPI_CROSS_KV )
			{
				f16* const L = (f16*)ldsWave;
				// column block -> what it is (uniform over the wave: 64 columns never straddle a head)
				int sel = 0, head = 0, layer = 0;
				if constexpr( EPI == EPI_QKV_ENC )
				{
					sel = n0 / d;
					head = ( n0 - sel * d ) >> 6;
				}
				if constexpr( EPI == EPI_CROSS_KV )
				{
					layer = n0 / ( 2 * d );
					const int c2 = n0 - layer * 2 * d;
					sel = c2 >= d ? 1 : 0;
					head = ( sel ? c2 - d : c2 ) >> 6;
				}
	#pragma unroll
				for( int i = 0; i < 2; i++ )
	#pragma unroll
					for( int j = 0; j < 2; j++ )
	#pragma unroll
						for( int r = 0; r < 16; r++ )
						{
							const int row = i * 32 + ( r & 3 ) + 8 * ( r >> 2 ) + 4 * hi;
							const int col = j * 32 + c;
							const float v = acc[ i ][ j ][ r ];
							f16 hv;
							if constexpr( EPI == EPI_F16_GELU )
								hv = gelu16( v + bias[ j ] );
							else if constexpr( EPI == EPI_QKV_ENC )
								hv = (f16)( v + bias[ j ] );
							else
								hv = sel ? (f16)( v + bias[ j ] ) : (f16)( v * a.scale );
							L[ row * 64 + ( ( ( col >> 3 ) ^ ( row & 7 ) ) << 3 ) + ( col & 7 ) ] = hv;
						}
				__builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront" );
				__builtin_amdgcn_wave_barrier();
				__builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront" );
				const int chunk = lane & 7;
	#pragma unroll
				for( int it = 0; it < 8; it++ )
				{
					const int row = it * 8 + ( lane >> 3 );
					const int m = m0 + row;
					const f16x8 v = *(const f16x8*)( L + row * 64 + ( ( chunk ^ ( row & 7 ) ) << 3 ) );
					const int n = n0 + chunk * 8;
					if( m >= a.M || n >= a.N ) continue;
					if constexpr( EPI == EPI_F16_GELU )
						*(f16x8*)( a.out16 + rowOffset( m, a.Mb, a.ldc, a.cBatchStride ) + n ) = v;
					else
					{
						const int b = m / a.T;
						const int t = m - b * a.T;
						if constexpr( EPI == EPI_QKV_ENC )
						{
							f16* const dst = sel == 0 ? a.q : a.k;
							*(f16x8*)( dst + ( ( (long long)b * a.H + head ) * a.T + t ) * HEAD_DIM + chunk * 8 ) = v;
						}
						else
						{
							f16* const dst = sel ? a.v : a.k;
							*(f16x8*)( dst + ( ( ( (long long)layer * a.B + b ) * a.H + head ) * a.T + t ) * HEAD_DIM + chunk * 8 ) = v;
						}
					}
				}
			}
			else
			{
				// FP32 outputs: 32 rows at a time
				float* const L = (float*)ldsWave;
				const int chunk = lane & 15;
	#pragma unroll
				for( int i = 0; i < 2; i++ )
				{
					if( i == 1 )
					{
						__builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront" );
						__builtin_amdgcn_wave_barrier();
						__builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront" );
					}
	#pragma unroll
					for( int j = 0; j < 2; j++ )
	#pragma unroll
						for( int r = 0; r < 16; r++ )
						{
							const int row = ( r & 3 ) + 8 * ( r >> 2 ) + 4 * hi;
							const int col = j * 32 + c;
							float v = acc[ i ][ j ][ r ] + bias[ j ];
							if constexpr( EPI == EPI_CONV2 ) v = (float)gelu16( v );
							L[ row * 64 + ( ( ( col >> 2 ) ^ ( row & 15 ) ) << 2 ) + ( col & 3 ) ] = v;
						}
					__builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront" );
					__builtin_amdgcn_wave_barrier();
					__builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront" );
					// everything a group of 4 chunks READS from memory first, then its stores (two groups per half: 16 + 8 registers
					// of operands in flight instead of 32 + 16)
	#pragma unroll
					for( int g4 = 0; g4 < 2; g4++ )
					{
						f32x4 ex[ 4 ];
						long long off[ 4 ];
	#pragma unroll
						for( int u = 0; u < 4; u++ )
						{
							const int row = ( g4 * 4 + u ) * 4 + ( lane >> 4 );
							int m = m0 + i * 32 + row;
							m = m < a.M ? m : a.M - 1;
							int n = n0 + chunk * 4;
							n = n < a.N ? n : a.N - 4;
							if constexpr( EPI == EPI_F32 )
							{
								off[ u ] = rowOffset( m, a.Mb, a.ldc, a.cBatchStride ) + n;
								ex[ u ] = a.res ? *(const f32x4*)( a.res + off[ u ] ) : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
							}
							else
							{
								const int b = m / a.Mb;
								off[ u ] = (long long)m * a.ldc + n;
								ex[ u ] = *(const f32x4*)( a.pe + (long long)( m - b * a.Mb ) * a.N + n );
							}
						}
	#pragma unroll
						for( int u = 0; u < 4; u++ )
						{
							const int row = ( g4 * 4 + u ) * 4 + ( lane >> 4 );
							const int m = m0 + i * 32 + row;
							const int n = n0 + chunk * 4;
							if( m >= a.M || n >= a.N ) continue;
							const f32x4 v = *(const f32x4*)( L + row * 64 + ( ( chunk ^ ( row & 15 ) ) << 2 ) );
							f32x4 o;
	#pragma unroll
							for( int e = 0; e < 4; e++ ) o[ e ] = EPI == EPI_F32 ? v[ e ] + ex[ u ][ e ] : ex[ u ][ e ] + v[ e ];
							*(f32x4*)( a.out32 + off[ u ] ) = o;
						}
					}
				}
			}
		}

		template<int EPI, class C, bool WIDE = false>
		__global__ void __launch_bounds__( C::NT, C::MINW ) gemmTiled( const GemmArgs a )
		{
			constexpr int BM = C::BM, BN = C::BN, BK = C::BK, LDS_STRIDE = C::STRIDE;
			extern __shared__ __attribute__( ( aligned( 16 ) ) ) unsigned char smem[];
			f16* const lds = (f16*)smem;

			const int tid = threadIdx.x;
			const int lane = tid & 63;
			const int wave = tid >> 6;
			const int wm = wave / C::WAVES_N, wn = wave % C::WAVES_N;

			const int tilesN = ( a.N + BN - 1 ) / BN;
			// XCD-aware, bijective block remap (each XCD gets a contiguous range of linear tile ids)
			int lin;
			{
				const int nb = gridDim.x, bid = blockIdx.x;
				const int q = nb >> 3, r = nb & 7;
				const int xcd = bid & 7, idx = bid >> 3;
				lin = ( xcd < r ? xcd * ( q + 1 ) : r * ( q + 1 ) + ( xcd - r ) * q ) + idx;
			}
			// Walk order inside an XCD's range. Row-major (tm = lin / tilesN) makes the ~32 (256x256) or ~96 (128x128) tiles an
			// XCD has in flight share ONE A tile and sweep that many different W tiles through a 4 MiB L2, so W is re-read from
			// the fabric once per M tile row (measured 8.3 GB for 0.12 GB of operands on the cross-KV product,
			// profiles/r01_pmc_hbm_traffic.csv). Bands of groupM M tiles, walked column by column, keep the band's A rows
			// (groupM x BM x K halves) resident while every W tile is fetched once per band and shared by groupM tiles.
			int tm, tn;
			if( a.groupM > 1 )
			{
				const int tilesM = ( a.M + BM - 1 ) / BM;
				const int perBand = a.groupM * tilesN;
				const int band = lin / perBand;
				const int first = band * a.groupM;
				const int rows = min( tilesM - first, a.groupM );
				const int r = lin - band * perBand;
				tm = first + r % rows;
				tn = r / rows;
			}
			else
			{
				tm = lin / tilesN;
				tn = lin - tm * tilesN;
			}

			if constexpr( C::GL )
			{
				// ---- direct-to-LDS pipeline: one barrier per K step, tile kt+1 lands while tile kt is multiplied ----
				const f16* gA[ C::IA ];
				const f16* gW[ C::IW ];
				const int rIn = lane / C::CPR, cPhys = lane % C::CPR;
#pragma unroll
				for( int i = 0; i < C::IA; i++ )
				{
					const int row = ( wave * C::IA + i ) * C::RPI + rIn;
					const int c = cPhys ^ ( ( row / C::RPB ) % C::CPR );
					int m = tm * BM + row;
					m = m < a.M ? m : a.M - 1;
					gA[ i ] = a.A + rowOffset( m, a.Mb, a.lda, a.aBatchStride ) + c * 8;
				}
#pragma unroll
				for( int i = 0; i < C::IW; i++ )
				{
					const int row = ( wave * C::IW + i ) * C::RPI + rIn;
					const int c = cPhys ^ ( ( row / C::RPB ) % C::CPR );
					int n = tn * BN + row;
					n = n < a.N ? n : a.N - 1;
					gW[ i ] = a.W + (long long)n * a.K + c * 8;
				}
				f32x16 acc[ C::TI ][ C::TJ ];
#pragma unroll
				for( int i = 0; i < C::TI; i++ )
#pragma unroll
					for( int j = 0; j < C::TJ; j++ )
#pragma unroll
						for( int r = 0; r < 16; r++ )
							acc[ i ][ j ][ r ] = 0.0f;
				const int nk = a.K / BK;
				const int fragRow = lane & 31;
				const int fragC = lane >> 5;
				typedef __attribute__( ( address_space( 3 ) ) ) void* LdsPtr;
				typedef const __attribute__( ( address_space( 1 ) ) ) void* GlobalPtr;
				// the LDS-DMA instructions p0 .. p1-1 of tile kt (A pieces first, then W pieces)
				auto issuePieces = [ & ]( int kt, int buf, int p0, int p1 )
				{
					f16* const dstA = lds + buf * C::STAGE + wave * C::IA * C::RPI * BK;
					f16* const dstW = lds + buf * C::STAGE + C::A_HALFS + wave * C::IW * C::RPI * BK;
					const int ko = kt * BK;
					if constexpr( C::FRAGPF )
					{
						// Issued as assembly: hipcc models the builtin as a FLAT access that may touch LDS and, while one is in
						// flight, turns every LDS wait of the wave into lgkmcnt(0) -- the fragment prefetch below needs counted
						// waits. The loads are ordered by the explicit vmcnt waits + barriers of the K loop.
						const unsigned baseA = __builtin_amdgcn_readfirstlane( (unsigned)(size_t)(LdsPtr)dstA );
						const unsigned baseW = __builtin_amdgcn_readfirstlane( (unsigned)(size_t)(LdsPtr)dstW );
	#pragma unroll
						for( int i = 0; i < C::IA; i++ )
							if( i >= p0 && i < p1 )
								ldsDma16( gA[ i ] + ko, baseA + i * C::RPI * BK * 2 );
	#pragma unroll
						for( int i = 0; i < C::IW; i++ )
							if( C::IA + i >= p0 && C::IA + i < p1 )
								ldsDma16( gW[ i ] + ko, baseW + i * C::RPI * BK * 2 );
						return;
					}
#pragma unroll
					for( int i = 0; i < C::IA; i++ )
						__builtin_amdgcn_global_load_lds( (GlobalPtr)( gA[ i ] + ko ), (LdsPtr)( dstA + i * C::RPI * BK ), 16, 0, 0 );
#pragma unroll
					for( int i = 0; i < C::IW; i++ )
						__builtin_amdgcn_global_load_lds( (GlobalPtr)( gW[ i ] + ko ), (LdsPtr)( dstW + i * C::RPI * BK ), 16, 0, 0 );
				};
				constexpr int NB = C::NBUF;
				constexpr int PER_TILE = C::IA + C::IW;	  // LDS-DMA instructions of one tile per wave
				auto issue = [ & ]( int kt, int buf ) { issuePieces( kt, buf, 0, PER_TILE ); };
	#pragma unroll
				for( int p = 0; p < NB - 1; p++ )
					if( p < nk ) issue( p, p );
				for( int kt = 0; kt < nk; kt++ )
				{
					const int buf = kt % NB;
					if constexpr( NB == 2 )
					{
						asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
						__syncthreads();
					}
					else
					{
						// tile kt must have landed; the NB - 2 tiles behind it may stay in flight (they were issued later and
						// complete in order). A plain __syncthreads() would drain them: raw barrier.
						if( kt + NB - 2 < nk )
							asm volatile( "s_waitcnt vmcnt(%0)" ::"n"( ( NB - 2 ) * PER_TILE ) : "memory" );
						else
							asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
						__builtin_amdgcn_s_barrier();
					}
					if( kt + NB - 1 < nk ) issue( kt + NB - 1, ( kt + NB - 1 ) % NB );
					const f16* const ldsA = lds + buf * C::STAGE;
					const f16* const ldsW = ldsA + C::A_HALFS;
					if constexpr( C::FRAGPF )
					{
						f16x8 fa[ 2 ][ C::TI ], fb[ 2 ][ C::TJ ];
						auto readFrags = [ & ]( auto set, int ks )
						{
							constexpr int S = decltype( set )::value;
	#pragma unroll
							for( int i = 0; i < C::TI; i++ )
								fa[ S ][ i ] = *(const f16x8*)( ldsA + glOffset<C>( wm * 32 * C::TI + i * 32 + fragRow, ks * 2 + fragC ) );
	#pragma unroll
							for( int j = 0; j < C::TJ; j++ )
								fb[ S ][ j ] = *(const f16x8*)( ldsW + glOffset<C>( wn * 32 * C::TJ + j * 32 + fragRow, ks * 2 + fragC ) );
						};
						auto mfmas = [ & ]( auto set )
						{
							constexpr int S = decltype( set )::value;
	#pragma unroll
							for( int i = 0; i < C::TI; i++ )
	#pragma unroll
								for( int j = 0; j < C::TJ; j++ )
									acc[ i ][ j ] = __builtin_amdgcn_mfma_f32_32x32x16_f16( fa[ S ][ i ], fb[ S ][ j ], acc[ i ][ j ], 0, 0, 0 );
						};
						using S0 = std::integral_constant<int, 0>;
						using S1 = std::integral_constant<int, 1>;
						static_assert( ( BK / 16 ) % 2 == 0, "fragment prefetch walks the k-substeps in pairs" );
						readFrags( S0{}, 0 );
	#pragma unroll
						for( int ks = 0; ks < BK / 16; ks += 2 )
						{
							// the scheduling fences keep hipcc from sinking the reads back below the MFMAs to save registers
							readFrags( S1{}, ks + 1 );
							__builtin_amdgcn_sched_barrier( 0 );
							mfmas( S0{} );
							__builtin_amdgcn_sched_barrier( 0 );
							if( ks + 2 < BK / 16 ) readFrags( S0{}, ks + 2 );
							__builtin_amdgcn_sched_barrier( 0 );
							mfmas( S1{} );
							__builtin_amdgcn_sched_barrier( 0 );
						}
					}
					else
					{
	#pragma unroll
					for( int ks = 0; ks < BK / 16; ks++ )
					{
						f16x8 fa[ C::TI ], fb[ C::TJ ];
	#pragma unroll
						for( int i = 0; i < C::TI; i++ )
							fa[ i ] = *(const f16x8*)( ldsA + glOffset<C>( wm * 32 * C::TI + i * 32 + fragRow, ks * 2 + fragC ) );
	#pragma unroll
						for( int j = 0; j < C::TJ; j++ )
							fb[ j ] = *(const f16x8*)( ldsW + glOffset<C>( wn * 32 * C::TJ + j * 32 + fragRow, ks * 2 + fragC ) );
	#pragma unroll
						for( int i = 0; i < C::TI; i++ )
	#pragma unroll
							for( int j = 0; j < C::TJ; j++ )
								acc[ i ][ j ] = __builtin_amdgcn_mfma_f32_32x32x16_f16( fa[ i ], fb[ j ], acc[ i ][ j ], 0, 0, 0 );
					}
					}
				}
				if constexpr( WIDE )
				{
					// V of the encoder (fragment-major, already 8-byte stores of 4 keys) keeps the direct path; a wave's 64 columns are one head
					const bool vPart = EPI == EPI_QKV_ENC && ( tn * BN + wn * 64 ) >= 2 * a.H * HEAD_DIM;
					__syncthreads();	  // every wave is done reading the operand tiles: LDS is free
					if( !vPart )
					{
						tileEpilogueWide<EPI, C>( a, acc, tm, tn, wm, wn, lane, smem + wave * 8192 );
						return;
					}
				}
				tileEpilogue<EPI, C>( a, acc, tm, tn, wm, wn, lane );
			}
			else
			{
			// global -> register staging: CA / CW chunks of 16 bytes per thread
			const f16* gA[ C::CA ];
			const f16* gW[ C::CW ];
			int offA[ C::CA ], offW[ C::CW ];
#pragma unroll
			for( int i = 0; i < C::CA; i++ )
			{
				const int c = tid + i * C::NT;
				const int row = c / C::CPR;
				const int kc = ( c % C::CPR ) * 8;
				int m = tm * BM + row;
				m = m < a.M ? m : a.M - 1;
				gA[ i ] = a.A + rowOffset( m, a.Mb, a.lda, a.aBatchStride ) + kc;
				offA[ i ] = row * LDS_STRIDE + kc;
			}
#pragma unroll
			for( int i = 0; i < C::CW; i++ )
			{
				const int c = tid + i * C::NT;
				const int row = c / C::CPR;
				const int kc = ( c % C::CPR ) * 8;
				int n = tn * BN + row;
				n = n < a.N ? n : a.N - 1;
				gW[ i ] = a.W + (long long)n * a.K + kc;
				offW[ i ] = C::A_HALFS + row * LDS_STRIDE + kc;
			}

			f32x16 acc[ 2 ][ 2 ];
#pragma unroll
			for( int i = 0; i < 2; i++ )
#pragma unroll
				for( int j = 0; j < 2; j++ )
#pragma unroll
					for( int r = 0; r < 16; r++ )
						acc[ i ][ j ][ r ] = 0.0f;

			// Register prefetch, PF tiles deep: while tile kt is consumed from LDS, tile kt+1 sits in a register set (written
			// to the other LDS buffer after the MFMAs) and, with PF == 2, the loads of tile kt+2 are already in flight in the
			// second set. The loop is unrolled by two so that the sets are statically indexed.
			u32x4 ra[ 2 ][ C::CA ], rw[ 2 ][ C::CW ];
			const int nk = a.K / BK;
			const int fragRow = lane & 31;
			const int fragK = ( lane >> 5 ) * 8;

			auto loadTile = [ & ]( auto set, int kt )
			{
				constexpr int S = decltype( set )::value;
				const int ko = kt * BK;
#pragma unroll
				for( int i = 0; i < C::CA; i++ ) ra[ S ][ i ] = *(const u32x4*)( gA[ i ] + ko );
#pragma unroll
				for( int i = 0; i < C::CW; i++ ) rw[ S ][ i ] = *(const u32x4*)( gW[ i ] + ko );
			};
			auto storeTile = [ & ]( auto set, int buf )
			{
				constexpr int S = decltype( set )::value;
				f16* const dst = lds + buf * C::STAGE;
#pragma unroll
				for( int i = 0; i < C::CA; i++ ) *(u32x4*)( dst + offA[ i ] ) = ra[ S ][ i ];
#pragma unroll
				for( int i = 0; i < C::CW; i++ ) *(u32x4*)( dst + offW[ i ] ) = rw[ S ][ i ];
			};
			auto compute = [ & ]( int buf )
			{
				const f16* const ldsA = lds + buf * C::STAGE;
				const f16* const ldsW = ldsA + C::A_HALFS;
#pragma unroll
				for( int ks = 0; ks < BK / 16; ks++ )
				{
					f16x8 fa[ 2 ], fb[ 2 ];
#pragma unroll
					for( int i = 0; i < 2; i++ )
					{
						fa[ i ] = *(const f16x8*)( ldsA + ( wm * 64 + i * 32 + fragRow ) * LDS_STRIDE + ks * 16 + fragK );
						fb[ i ] = *(const f16x8*)( ldsW + ( wn * 64 + i * 32 + fragRow ) * LDS_STRIDE + ks * 16 + fragK );
					}
#pragma unroll
					for( int i = 0; i < 2; i++ )
#pragma unroll
						for( int j = 0; j < 2; j++ )
							acc[ i ][ j ] = __builtin_amdgcn_mfma_f32_32x32x16_f16( fa[ i ], fb[ j ], acc[ i ][ j ], 0, 0, 0 );
				}
			};
			using Set0 = std::integral_constant<int, 0>;
			using Set1 = std::integral_constant<int, 1>;

			if constexpr( C::PF == 2 )
			{
				loadTile( Set0{}, 0 );
				if( nk > 1 ) loadTile( Set1{}, 1 );
				storeTile( Set0{}, 0 );
				__syncthreads();
				for( int kt = 0; kt < nk; kt += 2 )
				{
					// even step: tile kt in LDS buffer 0, tile kt+1 in register set 1
					if( kt + 2 < nk ) loadTile( Set0{}, kt + 2 );
					compute( 0 );
					if( kt + 1 < nk ) storeTile( Set1{}, 1 );
					__syncthreads();
					if( kt + 1 >= nk ) break;
					// odd step: tile kt+1 in LDS buffer 1, tile kt+2 in register set 0
					if( kt + 3 < nk ) loadTile( Set1{}, kt + 3 );
					compute( 1 );
					if( kt + 2 < nk ) storeTile( Set0{}, 0 );
					__syncthreads();
				}
			}
			else
			{
				loadTile( Set0{}, 0 );
				storeTile( Set0{}, 0 );
				__syncthreads();
				for( int kt = 0; kt < nk; kt++ )
				{
					const int cur = kt & 1;
					if( kt + 1 < nk ) loadTile( Set0{}, kt + 1 );
					compute( cur );
					if( kt + 1 < nk ) storeTile( Set0{}, cur ^ 1 );
					__syncthreads();
				}
			}

			tileEpilogue<EPI, C>( a, acc, tm, tn, wm, wn, lane );
			}
		}
	}	// namespace

	template<int EPI, class C = CfgDefault>
	static int launchTiledT( const GemmArgs& a, hipStream_t stream )
	{
		GemmArgs b = a;
		if( b.groupM == 0 ) b.groupM = ( g_tuning & TUNE_GEMM_GROUP_M ) ? ( C::BM >= 256 ? 4 : 8 ) : 1;
		const int tilesM = ( b.M + C::BM - 1 ) / C::BM, tilesN = ( b.N + C::BN - 1 ) / C::BN;
		// tileEpilogueWide is written for the direct-to-LDS configurations with 64x64 wave tiles
		constexpr bool canWide = C::GL && C::TI == 2 && C::TJ == 2 &&
			( EPI == EPI_F32 || EPI == EPI_F16_GELU || EPI == EPI_CONV2 || EPI == EPI_QKV_ENC || EPI == EPI_CROSS_KV );
		if constexpr( canWide )
			if( wideEpilogueOk( a, EPI ) )
			{
				b.wideEpi = t_gemmWideEpi = 1;
				return launchLds<gemmTiled<EPI, C, true>>( dim3( tilesM * tilesN ), dim3( C::NT ), C::LDS_BYTES, stream, b );
			}
		b.wideEpi = t_gemmWideEpi = 0;
		return launchLds<gemmTiled<EPI, C, false>>( dim3( tilesM * tilesN ), dim3( C::NT ), C::LDS_BYTES, stream, b );
	}

	// The configurations an epilogue is built with: CAN_BIG = the 256x256x64 tiles too, CAN_PF = the fragment prefetch too
	template<int EPI, bool CAN_BIG, bool CAN_PF>
	static int launchTiledE( const GemmArgs& a, bool big, hipStream_t stream )
	{
		const bool gl = ( g_tuning & TUNE_GEMM_GL ) != 0;
		const bool pf = gl && ( g_tuning & TUNE_GEMM_FRAGPF ) != 0;
		if constexpr( CAN_BIG && CAN_PF )
			if( pf && big ) return launchTiledT<EPI, CfgGlBigPf>( a, stream );
		if constexpr( CAN_PF )
			if( pf ) return launchTiledT<EPI, CfgGlPf>( a, stream );
		if constexpr( CAN_BIG )
			if( gl && big ) return launchTiledT<EPI, CfgGlBig>( a, stream );
		if( gl ) return launchTiledT<EPI, CfgGl>( a, stream );
		if constexpr( CAN_BIG )
			if( big ) return launchTiledT<EPI, CfgBig>( a, stream );
		return launchTiledT<EPI>( a, stream );
	}

	// the epilogues built with the 256x256x64 tiles too; the others take 128x128x32 whatever `big` says
	static constexpr bool bigTiles( int epi ) { return epi == EPI_F32 || epi == EPI_F16_GELU || epi == EPI_QKV_ENC || epi == EPI_CROSS_KV; }
	bool tiledBigEpilogue( int epi ) { return bigTiles( epi ); }

	int launchTiled( const GemmArgs& a, bool big, hipStream_t stream )
	{
		switch( a.epi )
		{
		case EPI_F32: return launchTiledE<EPI_F32, bigTiles( EPI_F32 ), true>( a, big, stream );
		case EPI_F16_GELU: return launchTiledE<EPI_F16_GELU, bigTiles( EPI_F16_GELU ), true>( a, big, stream );
		case EPI_CONV2: return launchTiledE<EPI_CONV2, bigTiles( EPI_CONV2 ), true>( a, big, stream );
		case EPI_QKV_ENC: return launchTiledE<EPI_QKV_ENC, bigTiles( EPI_QKV_ENC ), true>( a, big, stream );
		case EPI_CROSS_KV: return launchTiledE<EPI_CROSS_KV, bigTiles( EPI_CROSS_KV ), true>( a, big, stream );
		case EPI_QKV_DEC: return launchTiledE<EPI_QKV_DEC, bigTiles( EPI_QKV_DEC ), false>( a, big, stream );
		case EPI_Q_DEC: return launchTiledE<EPI_Q_DEC, bigTiles( EPI_Q_DEC ), false>( a, big, stream );
		}
		setError( "gemm: unknown epilogue" );
		return -1;
	}

	// Tile-shape experiments on the plain FP32 epilogue (tools/gemm_probe.py): variant -> configuration
	int launchTiledVariant( const GemmArgs& a, int variant, hipStream_t stream )
	{
		switch( variant )
		{
		case 25: return launchTiledT<EPI_F32, TileCfg<256, 256, 64, 4, 1, true, 2, 2, 2, 1>>( a, stream );	   // the 16-wave kernel of round 2 (products below gemmTiled8's threshold)
		case 26: return launchTiledT<EPI_F32, TileCfg<128, 128, 32, 3, 1, true, 2, 2, 2, 1>>( a, stream );
		case 2: return launchTiledT<EPI_F32, TileCfg<128, 128, 32, 3, 1>>( a, stream );	   // register-staged 128x128x32: what wh_debug_probe checks every variant against
#ifdef WH_PROBES
		// Everything below exists for tools/*probe*: tile-shape experiments (all correct). The shipped objects do not contain them: build with
		// WH_PROBES=1 python -m whisper_amd.build --force to get them back. (The ABLATIONS of rounds 2-4 -- kernels with loads, fragment reads,
		// MFMAs or stores removed to see what the rest costs: profiles/r02_gemm_kloop_ablation.txt, r03_gemm8_ablation.txt, r04_gemm4_probe.txt --
		// lived in the production kernels' source as compile-time branches until round 5; they are in the history up to commit 7317048.)
		case 27: return launchTiledT<EPI_F32, TileCfg<256, 256, 32, 4, 1, true, 2, 2, 3, 1>>( a, stream );
		case 20: return launchTiledT<EPI_F32, TileCfg<256, 256, 32, 4, 1, true, 2, 2, 3>>( a, stream );
		case 21: return launchTiledT<EPI_F32, TileCfg<256, 256, 32, 4, 1, true, 2, 2, 4>>( a, stream );
		case 22: return launchTiledT<EPI_F32, TileCfg<256, 128, 64, 2, 1, true, 2, 2, 3>>( a, stream );
		case 23: return launchTiledT<EPI_F32, TileCfg<256, 256, 32, 4, 1, true, 2, 2, 2>>( a, stream );
		case 24: return launchTiledT<EPI_F32, TileCfg<128, 256, 64, 2, 1, true, 2, 2, 3>>( a, stream );
		case 10: return launchTiledT<EPI_F32, TileCfg<128, 128, 64, 2, 1, true>>( a, stream );
		case 11: return launchTiledT<EPI_F32, TileCfg<128, 128, 32, 3, 1, true>>( a, stream );
		case 12: return launchTiledT<EPI_F32, TileCfg<256, 256, 64, 4, 1, true>>( a, stream );
		case 13: return launchTiledT<EPI_F32, TileCfg<256, 128, 64, 2, 1, true>>( a, stream );
		case 14: return launchTiledT<EPI_F32, TileCfg<256, 128, 32, 2, 1, true, 4, 2>>( a, stream );
		case 15: return launchTiledT<EPI_F32, TileCfg<256, 128, 64, 1, 1, true, 4, 2>>( a, stream );
		case 16: return launchTiledT<EPI_F32, TileCfg<256, 256, 64, 2, 1, true, 4, 2>>( a, stream );
		case 17: return launchTiledT<EPI_F32, TileCfg<256, 256, 32, 2, 1, true, 4, 2>>( a, stream );
		case 18: return launchTiledT<EPI_F32, TileCfg<128, 256, 32, 2, 1, true, 2, 4>>( a, stream );
		case 0: return launchTiledT<EPI_F32, TileCfg<128, 128, 64, 2, 2>>( a, stream );
		case 9: return launchTiledT<EPI_F32, TileCfg<128, 128, 32, 3, 1>>( a, stream );
		case 1: return launchTiledT<EPI_F32, TileCfg<128, 128, 64, 2, 1>>( a, stream );
		case 3: return launchTiledT<EPI_F32, TileCfg<256, 128, 64, 2, 1>>( a, stream );
		case 4: return launchTiledT<EPI_F32, TileCfg<256, 128, 64, 2, 2>>( a, stream );
		case 5: return launchTiledT<EPI_F32, TileCfg<256, 128, 32, 4, 1>>( a, stream );
		case 6: return launchTiledT<EPI_F32, TileCfg<256, 256, 64, 4, 1>>( a, stream );
		case 7: return launchTiledT<EPI_F32, TileCfg<128, 256, 64, 2, 1>>( a, stream );
		case 8: return launchTiledT<EPI_F32, TileCfg<256, 256, 32, 4, 1>>( a, stream );
#endif
		}
#ifdef WH_PROBES
		setError( "gemm: unknown variant" );
#else
		setError( "gemm: probe variants are not part of this build (WH_PROBES=1 python -m whisper_amd.build --force)" );
#endif
		return -1;
	}
}
