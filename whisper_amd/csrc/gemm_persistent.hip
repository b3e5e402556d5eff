// gemmTiled8 and gemmTiled4: the encoder's NT GEMM for batches several clips deep, PERSISTENT -- one workgroup per CU walks its share of the
// 256x256x64 output tiles (FP16 x FP16 -> FP32 on MFMA, fused epilogues). Eight waves in four phases per K tile, or four waves with one barrier
// per K tile; both hand-scheduled, both described at the kernel. They share the epilogues of their interior tiles (epilogueFast4), which is
// why they share a unit.
#include "gemm_device.h"
#include "gemm_launch.h"
#include <stdlib.h>
#include <atomic>

namespace wh
{
	namespace
	{

		// ---------------------------------------------------------------------------------------------------------------
		// gemmTiled8: the encoder GEMM for batches several clips deep. PERSISTENT: one workgroup per CU walks its share of the
		// 256x256 output tiles. EIGHT waves as 2 (M) x 4 (N), a wave owns 128 x 64 outputs = 4 x 2 MFMA 32x32x16 tiles (24
		// fragment reads per 32 MFMAs; the 16-wave 64x64 layout of gemmTiled reads 16 per 16), both operands global -> LDS
		// directly in full 128-byte lines, XOR-swizzled source, two 64 KiB K-tile buffers + 32 KiB of epilogue staging = all
		// 160 KiB of a CU. What differs from gemmTiled is the SCHEDULE (cdna_hip_programming.md section 5, T3+T4):
		//   * a K tile is four phases, one 64x32 quadrant of the wave's outputs each (8 MFMAs = 256 matrix-pipe cycles):
		//       phase    fragments read from LDS        MFMAs          staged global -> LDS (1 KiB per instruction and wave)
		//       1        a0 (8 reads), b0 (4 reads)     a0 x b0        --
		//       2        b1 (4)                         a0 x b1        A rows   0..127 of K tile t+1 (2)
		//       3        a1 (8)                         a1 x b1        A rows 128..255 of K tile t+1 (2)
		//       4        --                             a1 x b0        W tile (256 rows) of K tile t+2 (4)
		//     every phase is  { ds_reads, LDS-DMA issue } s_barrier { MFMAs } s_barrier;
		//   * the two wave rows run ONE barrier apart (the waves of row 1 execute an extra s_barrier before the loop, those of
		//     row 0 after it): on every SIMD one wave is in its MFMA segment while the other reads fragments and issues DMA,
		//     so the matrix pipe never waits for a barrier, an LDS round trip or a DMA issue slot -- as long as a read/issue
		//     segment fits under 256 cycles, which is why the eight DMA instructions of a K tile are spread over three phases;
		//   * vmcnt never drops to 0 inside the loop: W is requested a whole K tile ahead (phase 4 of tile t for t+2), A as soon
		//     as its buffer half is dead (phases 2 and 3 of tile t for t+1); the waits sit at the end of phase 4's issue segment
		//     (vmcnt(6): W and the first A half of t+1) and of its MFMA segment (vmcnt(4): the second A half), so 24 .. 64 KiB per
		//     CU are in flight at any time and a DMA has 3 (A rows 128..), 4 (A rows 0..) or 8 (W) barrier intervals to land.
		//     Waiting per half tile three intervals after its issue (the first version) kept 16 .. 32 KiB in flight and was
		//     latency-bound at 54 GB/s per CU (profiles/r03_gemm8_ablation.txt);
		//   * DMA addresses are SGPR base (advanced per K tile on the scalar unit) + a per-lane 32-bit byte offset that never
		//     changes: no vector ALU work per instruction;
		//   * the NEXT tile's first operands are requested before this tile's epilogue starts, and the epilogue goes through its
		//     own 4 KiB per wave, so a tile's stores drain under the next tile's K loop and its first-tile latency under the epilogue.
		// Hazards (interval = barrier to barrier, K tile t occupies intervals 0..7 of wave row 0 and 1..8 of row 1):
		//   RAW  operands of tile t+1: W issued in -2 / -1 (row 0 / row 1), A rows 0.. in 2 / 3, A rows 128.. in 4 / 5. Row 0 reads
		//        W and A rows 0.. from interval 8, row 1 reads W and A rows 128.. from 9. Waits: vmcnt(6) at the end of 6 / 7
		//        (W, A rows 0..), vmcnt(4) at the end of 7 / 8 (A rows 128..); each is followed by a barrier both rows pass
		//        before the first read.
		//   WAR  buffer (t+1)&1 was last read by tile t-1: its W in interval -5 (row 1, phase 2), A rows 0.. in -4 (row 0, phase
		//        3), A rows 128.. in -3 (row 1, phase 3); those reads are retired by the MFMAs of the following interval, and the
		//        first DMA into each region is issued in -2, 2 and 4: at least two barriers later.
		struct Cfg8
		{
			static constexpr int BM = 256, BN = 256, BK = 64, NT = 512, TI = 4, TJ = 2;
			static constexpr int A_HALFS = BM * BK, STAGE = ( BM + BN ) * BK;	   // halfs per K-tile buffer: A tile, then W tile
			static constexpr int EPI_OFFSET = 2 * STAGE * 2;					   // bytes: the epilogue staging starts behind the two buffers
			static constexpr int EPI_PER_WAVE = 4096;
			static constexpr int LDS_BYTES = EPI_OFFSET + 8 * EPI_PER_WAVE;		   // 160 KiB
		};

		// One 32-row x 64-column block of a wave's outputs (MFMA tiles c0 = columns 0..31, c1 = 32..63 of the block) through 4 KiB of
		// LDS, leaving as 16-byte stores along the rows of the destination: the arithmetic of tileEpilogue / tileEpilogueWide per
		// element, FP16 outputs in one pass ([32][64] halfs), FP32 outputs in two ([16][64] floats each), 16-byte chunk index XORed
		// with the row so that the column-wise writes and the row-wise reads are both conflict free. m0 / n0 = first row / column.
		// Preconditions as for tileEpilogueWide (a.wideEpi). Residual / positional rows are requested before the LDS round trip.
		template<int EPI>
		__device__ __forceinline__ void epilogueBlock32x64( const GemmArgs& a, const f32x16& c0, const f32x16& c1, int m0, int n0, int lane, unsigned char* ldsWave )
		{
			const int hi = lane >> 5, c = lane & 31;
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
				const int d = a.H * HEAD_DIM;
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
				for( int j = 0; j < 2; j++ )
	#pragma unroll
					for( int r = 0; r < 16; r++ )
					{
						const int row = ( r & 3 ) + 8 * ( r >> 2 ) + 4 * hi;
						const int col = j * 32 + c;
						const float v = j == 0 ? c0[ r ] : c1[ r ];
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
				for( int it = 0; it < 4; it++ )
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
				__builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront" );
				__builtin_amdgcn_wave_barrier();
				__builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront" );
			}
			else
			{
				static_assert( EPI == EPI_F32 || EPI == EPI_CONV2, "FP32 block epilogue" );
				float* const L = (float*)ldsWave;
				const int chunk = lane & 15;
				// everything the block READS from memory first: 2 halves x 4 rows x 16 bytes per lane
				f32x4 ex[ 2 ][ 4 ];
				long long off[ 2 ][ 4 ];
	#pragma unroll
				for( int hh = 0; hh < 2; hh++ )
	#pragma unroll
					for( int u = 0; u < 4; u++ )
					{
						int m = m0 + hh * 16 + u * 4 + ( lane >> 4 );
						m = m < a.M ? m : a.M - 1;
						int n = n0 + chunk * 4;
						n = n < a.N ? n : a.N - 4;
						if constexpr( EPI == EPI_F32 )
						{
							off[ hh ][ u ] = rowOffset( m, a.Mb, a.ldc, a.cBatchStride ) + n;
							ex[ hh ][ u ] = a.res ? *(const f32x4*)( a.res + off[ hh ][ u ] ) : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
						}
						else
						{
							const int b = m / a.Mb;
							off[ hh ][ u ] = (long long)m * a.ldc + n;
							ex[ hh ][ u ] = *(const f32x4*)( a.pe + (long long)( m - b * a.Mb ) * a.N + n );
						}
					}
	#pragma unroll
				for( int hh = 0; hh < 2; hh++ )
				{
	#pragma unroll
					for( int j = 0; j < 2; j++ )
	#pragma unroll
						for( int q = 0; q < 8; q++ )
						{
							const int r = hh * 8 + q;
							const int row = ( q & 3 ) + 8 * ( q >> 2 ) + 4 * hi;	  // within the 16-row half
							const int col = j * 32 + c;
							float v = ( j == 0 ? c0[ r ] : c1[ r ] ) + bias[ j ];
							if constexpr( EPI == EPI_CONV2 ) v = (float)gelu16( v );
							L[ row * 64 + ( ( ( col >> 2 ) ^ row ) << 2 ) + ( col & 3 ) ] = v;
						}
					__builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront" );
					__builtin_amdgcn_wave_barrier();
					__builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront" );
	#pragma unroll
					for( int u = 0; u < 4; u++ )
					{
						const int row = u * 4 + ( lane >> 4 );
						const int m = m0 + hh * 16 + row;
						const int n = n0 + chunk * 4;
						const f32x4 v = *(const f32x4*)( L + row * 64 + ( ( chunk ^ row ) << 2 ) );
						if( m >= a.M || n >= a.N ) continue;
						f32x4 o;
	#pragma unroll
						for( int e = 0; e < 4; e++ ) o[ e ] = EPI == EPI_F32 ? v[ e ] + ex[ hh ][ u ][ e ] : ex[ hh ][ u ][ e ] + v[ e ];
						*(f32x4*)( a.out32 + off[ hh ][ u ] ) = o;
					}
					__builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront" );
					__builtin_amdgcn_wave_barrier();
					__builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront" );
				}
			}
		}

		// The V columns of the encoder's Q/K/V product, straight from the accumulators: fragment-major V (vFragIndex) keeps the
		// keys k..k+3 and k+8..k+11 of one dimension in one 16-byte chunk, and a lane of the 32x32 accumulator tile holds
		// exactly rows 4 hi + 8 g + {0..3} of one column -- so each group g of 4 registers is one 8-byte half of a chunk, and
		// groups g, g+1 are one whole chunk when the first one's key is a multiple of 8 inside its 16-key block. The chunks of
		// a store instruction are consecutive in memory (lane = dimension, hi = chunk + 32): 1 KiB per wave and instruction.
		// Requires T % 4 == 0 (a group of 4 rows never straddles two sequences); m0 / n0 = first row / column of the
		// 32 x 64 block, n0 a multiple of 64 inside the V third of the columns.
		__device__ __forceinline__ void epilogueBlockV32x64( const GemmArgs& a, const f32x16& c0, const f32x16& c1, int m0, int n0, int lane )
		{
			const int hi = lane >> 5, dd = lane & 31;
			const int d = a.H * HEAD_DIM;
			const int head = ( n0 - 2 * d ) >> 6;
			const int b0 = m0 / a.T;	   // wave-uniform
			const long long perSeq = (long long)a.H * HEAD_DIM * a.Tpad;
			f16* const vHead = a.v + (long long)head * HEAD_DIM * a.Tpad;
			int bOf[ 4 ], tOf[ 4 ];
			bool ok[ 4 ];
	#pragma unroll
			for( int g = 0; g < 4; g++ )
			{
				const int m = m0 + 4 * hi + 8 * g;
				int t = m - b0 * a.T, b = b0;
				if( t >= a.T )	  // the block runs into the next sequence (or, for T < 32, further)
				{
					b = m / a.T;
					t = m - b * a.T;
				}
				bOf[ g ] = b;
				tOf[ g ] = t;
				ok[ g ] = m < a.M;
			}
	#pragma unroll
			for( int j = 0; j < 2; j++ )
			{
				const int n = n0 + j * 32 + dd;
				const float bias = ( a.bias && n < a.N ) ? a.bias[ n ] : 0.0f;
				f16x4 pk[ 4 ];
	#pragma unroll
				for( int g = 0; g < 4; g++ )
	#pragma unroll
					for( int e = 0; e < 4; e++ ) pk[ g ][ e ] = (f16)( ( j == 0 ? c0[ 4 * g + e ] : c1[ 4 * g + e ] ) + bias );
				if( n >= a.N ) continue;
				auto dst = [ & ]( int g ) -> f16*
				{
					const int t = tOf[ g ];
					return vHead + bOf[ g ] * perSeq + ( ( (long long)( t >> 4 ) * 2 + j ) * 64 + ( ( t >> 2 ) & 1 ) * 32 + dd ) * 8 + ( ( t >> 3 ) & 1 ) * 4;
				};
				// groups g and g + 1 are one 16-byte chunk when g's keys are the first half of their 16-key block and g + 1 belongs
				// to the same sequence (a block that runs into the next sequence restarts the key count: checked per pair)
				auto whole = [ & ]( int g ) { return ok[ g + 1 ] && bOf[ g + 1 ] == bOf[ g ] && ( ( tOf[ g ] >> 3 ) & 1 ) == 0; };
				auto store16 = [ & ]( int g )
				{
					f16x8 w;
	#pragma unroll
					for( int e = 0; e < 4; e++ )
					{
						w[ e ] = pk[ g ][ e ];
						w[ 4 + e ] = pk[ g + 1 ][ e ];
					}
					*(f16x8*)dst( g ) = w;
				};
				auto store8 = [ & ]( int g )
				{
					if( ok[ g ] ) *(f16x4*)dst( g ) = pk[ g ];
				};
				if( whole( 0 ) )
				{
					store16( 0 );
					if( whole( 2 ) )
						store16( 2 );
					else
					{
						store8( 2 );
						store8( 3 );
					}
				}
				else
				{
					store8( 0 );
					if( whole( 1 ) )
					{
						store16( 1 );
						store8( 3 );
					}
					else
					{
						store8( 1 );
						if( whole( 2 ) )
							store16( 2 );
						else
						{
							store8( 2 );
							store8( 3 );
						}
					}
				}
			}
		}

		// the interior-tile epilogue of both persistent kernels (defined with gemmTiled4 below)
		template<int EPI, bool HASRES, int FIRST = 0, int LAST = 16, int TJ = 4, bool AGPR = true, bool L16 = false, typename ACC>
		__device__ __forceinline__ void epilogueFast4( const GemmArgs& a, ACC& acc, int mW, int nW, int lane, unsigned char* stage );

		// MF16 (round 6, the default: option gemm_mf16): the K loop on v_mfma_f32_16x16x32_f16 instead of v_mfma_f32_32x32x16_f16 -- a quadrant is 4 x 2 tiles of
		// 16 x 16 over two k-halves of 32, the W fragment the srcB operand of four consecutive instructions; the same LDS image, the same 24 fragment reads per K
		// tile, the same 128 accumulator registers. The chip sustains more of this shape under its power limit (tools/mfma_order_probe.hip; the vendor library's
		// kernel uses it), and the SUMS ARE THE SAME BITS: the matrix cores add a k-block of 8 (one lane's 16 bytes) at a time in both shapes, and both kernels hand
		// them the k-blocks of a row in the same order (max |diff| = 0 against the 32x32x16 instance on every probed shape; the model-level identity test covers
		// it). Interior tiles leave through epilogueFast4's L16 form straight from the 16 x 16 tiles; edge tiles and the V third of the encoder's Q/K/V product are
		// first brought into the 32 x 32 register layout through the wave's staging area (convert16) and take the epilogues written for it.
		// Measured (profiles/r06_evidence/gemm_vendor_gap.txt): probe +3.4 .. 4.5 % on the encoder's shapes, the class in the model 0.379 -> 0.41 of the MFMA peak.
		template<int EPI, bool WIDE, bool MF16 = false>
		__global__ void __launch_bounds__( 512, 2 ) gemmTiled8( const GemmArgs a )
		{
			using C = Cfg8;
			constexpr int BM = C::BM, BN = C::BN, BK = C::BK;
			extern __shared__ __attribute__( ( aligned( 16 ) ) ) unsigned char smem[];
			f16* const lds = (f16*)smem;
			typedef __attribute__( ( address_space( 3 ) ) ) void* LdsPtr;

			const int tid = threadIdx.x;
			const int lane = tid & 63;
			const int wave = __builtin_amdgcn_readfirstlane( tid >> 6 );
			const int wr = wave >> 2, wc = wave & 3;

			// ---- this workgroup's tiles: XCD x (workgroup id % 8) owns a contiguous range of the band-walk order; its workgroups
			// take consecutive tiles of that range round by round, so the ~32 tiles an XCD has in flight are neighbours in the walk
			const int tilesM = ( a.M + BM - 1 ) / BM, tilesN = ( a.N + BN - 1 ) / BN;
			const int nTiles = tilesM * tilesN;
			const int gm = a.groupM;
			int linFirst, linEnd, linStep;
			{
				const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
				const int q = nTiles >> 3, r = nTiles & 7;
				const int start = xcd < r ? xcd * ( q + 1 ) : r * ( q + 1 ) + ( xcd - r ) * q;
				linEnd = start + ( xcd < r ? q + 1 : q );
				linFirst = start + idx;
				linStep = ( gridDim.x + 7 - xcd ) >> 3;	   // workgroups of this XCD
			}
			auto tileCoords = [ & ]( int lin, int& tm, int& tn )
			{
				if( gm > 1 )
				{
					const int perBand = gm * tilesN;
					const int band = lin / perBand;
					const int first = band * gm;
					const int rows = min( tilesM - first, gm );
					const int r = lin - band * perBand;
					tm = first + r % rows;
					tn = r / rows;
				}
				else
				{
					tm = lin / tilesN;
					tn = lin - tm * tilesN;
				}
			};

			// ---- LDS-DMA sources: a half tile is 128 rows x 128 bytes = 16 pieces of 8 rows, a wave owns pieces 2 wave, 2 wave + 1.
			// Lane l of a piece lands at row l / 8, physical 16-byte chunk l % 8, which must hold logical chunk (l % 8) ^ ((row >> 1) & 7).
			// offA / offW = byte offset of that chunk from a.A / a.W at k = 0 (the launcher guarantees they fit 32 bits).
			const int rIn = lane >> 3, cPhys = lane & 7;
			unsigned offA[ 2 ][ 2 ], offW[ 2 ][ 2 ];
			auto tileOffsets = [ & ]( int tm, int tn )
			{
	#pragma unroll
				for( int h = 0; h < 2; h++ )
	#pragma unroll
					for( int i = 0; i < 2; i++ )
					{
						const int row = h * 128 + ( wave * 2 + i ) * 8 + rIn;
						const int c = cPhys ^ ( ( row >> 1 ) & 7 );
						int m = tm * BM + row;
						m = m < a.M ? m : a.M - 1;
						offA[ h ][ i ] = (unsigned)( ( rowOffset( m, a.Mb, a.lda, a.aBatchStride ) + c * 8 ) * 2 );
						int n = tn * BN + row;
						n = n < a.N ? n : a.N - 1;
						offW[ h ][ i ] = (unsigned)( ( (long long)n * a.K + c * 8 ) * 2 );
					}
			};
			const unsigned ldsBase = __builtin_amdgcn_readfirstlane( (unsigned)(size_t)(LdsPtr)lds );
			// byte address of this wave's first piece of a half tile inside buffer 0: + buf * STAGE * 2, + (W ? A_HALFS * 2 : 0), + h * 16384
			const unsigned pieceBase = ldsBase + (unsigned)wave * 2048u;
			// part: 0 = W rows 0.., 1 = W rows 128.., 2 = A rows 0.., 3 = A rows 128..
			auto stage = [ & ]( int kt, auto part )
			{
				constexpr int P = decltype( part )::value;
				constexpr bool isW = P < 2;
				constexpr int h = P & 1;
				const unsigned dst = pieceBase + (unsigned)( kt & 1 ) * ( C::STAGE * 2 ) + ( isW ? C::A_HALFS * 2 : 0 ) + h * 16384;
				const f16* const base = ( isW ? a.W : a.A ) + kt * BK;
				if constexpr( isW )
					ldsDmaPair( base, offW[ h ][ 0 ], offW[ h ][ 1 ], dst );
				else
					ldsDmaPair( base, offA[ h ][ 0 ], offA[ h ][ 1 ], dst );
			};
			using PW0 = std::integral_constant<int, 0>;
			using PW1 = std::integral_constant<int, 1>;
			using PA0 = std::integral_constant<int, 2>;
			using PA1 = std::integral_constant<int, 3>;
			const int nk = a.K / BK;
			// first operands of a tile: K tile 0 into buffer 0 and the W tile of K tile 1 into buffer 1 (12 instructions per wave)
			auto stageFirst = [ & ]()
			{
				stage( 0, PW0{} );
				stage( 0, PW1{} );
				stage( 0, PA0{} );
				stage( 0, PA1{} );
				if( nk > 1 )
				{
					stage( 1, PW0{} );
					stage( 1, PW1{} );
				}
			};

			// ---- fragment reads: lane l reads row l & 31 of a 32-row tile, logical chunk 2 ks + (l >> 5), stored at chunk ^ ((row >> 1) & 7);
			// the tile origins are multiples of 32 rows, so the XOR term depends on the lane only
			const int x0 = ( lane >> 5 ) ^ ( ( lane >> 1 ) & 7 );
			int laneK[ 4 ];
	#pragma unroll
			for( int ks = 0; ks < 4; ks++ ) laneK[ ks ] = ( lane & 31 ) * BK + ( ( x0 ^ ( ks << 1 ) ) << 3 );
			// MF16: lane l reads row l & 15 of a 16-row tile, logical chunk 4 h + (l >> 4) of k-half h
			int laneK16[ 2 ];
#pragma unroll
			for( int h = 0; h < 2; h++ ) laneK16[ h ] = ( lane & 15 ) * BK + ( ( ( ( h << 2 ) + ( lane >> 4 ) ) ^ ( ( lane >> 1 ) & 7 ) ) << 3 );
			const int aRow0 = wr * 128, wRow0 = wc * 64;

			int tm, tn;
			int lin = linFirst;
			if( lin >= linEnd ) return;
			tileCoords( lin, tm, tn );
			tileOffsets( tm, tn );
			stageFirst();

			for( ;; )
			{
				f32x16 acc[ 4 ][ 2 ];
				f32x4 acc16[ MF16 ? 8 : 1 ][ MF16 ? 4 : 1 ];
				if constexpr( MF16 )
				{
	#pragma unroll
					for( int i = 0; i < 8; i++ )
	#pragma unroll
						for( int j = 0; j < 4; j++ )
	#pragma unroll
							for( int r = 0; r < 4; r++ ) acc16[ i ][ j ][ r ] = 0.0f;
				}
				else
				{
	#pragma unroll
					for( int i = 0; i < 4; i++ )
	#pragma unroll
						for( int j = 0; j < 2; j++ )
	#pragma unroll
							for( int r = 0; r < 16; r++ ) acc[ i ][ j ][ r ] = 0.0f;
				}
				// MF16: fa[ i' >> 1 ][ 2 ( i' & 1 ) + h ] = rows 16 i' of the half, k-half h; fb[ 2 j' + h ] = columns 16 j' of the 32, k-half h
				f16x8 fa[ 2 ][ 4 ], fb0[ 4 ], fb1[ 4 ];
				auto readA = [ & ]( const f16* bufA, int half )
				{
					if constexpr( MF16 )
					{
	#pragma unroll
						for( int ip = 0; ip < 4; ip++ )
	#pragma unroll
							for( int h = 0; h < 2; h++ )
								fa[ ip >> 1 ][ ( ( ip & 1 ) << 1 ) + h ] = *(const f16x8*)( bufA + ( aRow0 + half * 64 + ip * 16 ) * BK + laneK16[ h ] );
					}
					else
					{
	#pragma unroll
						for( int i = 0; i < 2; i++ )
	#pragma unroll
							for( int ks = 0; ks < 4; ks++ )
								fa[ i ][ ks ] = *(const f16x8*)( bufA + ( aRow0 + ( half * 2 + i ) * 32 ) * BK + laneK[ ks ] );
					}
				};
				auto readB = [ & ]( const f16* bufW, int j, f16x8( &fb )[ 4 ] )
				{
					if constexpr( MF16 )
					{
	#pragma unroll
						for( int jp = 0; jp < 2; jp++ )
	#pragma unroll
							for( int h = 0; h < 2; h++ ) fb[ ( jp << 1 ) + h ] = *(const f16x8*)( bufW + ( wRow0 + j * 32 + jp * 16 ) * BK + laneK16[ h ] );
					}
					else
					{
	#pragma unroll
						for( int ks = 0; ks < 4; ks++ ) fb[ ks ] = *(const f16x8*)( bufW + ( wRow0 + j * 32 ) * BK + laneK[ ks ] );
					}
				};
				auto quadrant = [ & ]( auto i0c, auto jc, const f16x8( &fb )[ 4 ] )
				{
					constexpr int i0 = decltype( i0c )::value, j = decltype( jc )::value;
					__builtin_amdgcn_s_setprio( 1 );
					if constexpr( MF16 )
					{
	#pragma unroll
						for( int h = 0; h < 2; h++ )
	#pragma unroll
							for( int jp = 0; jp < 2; jp++ )
	#pragma unroll
								for( int ip = 0; ip < 4; ip++ )
									acc16[ 2 * i0 + ip ][ 2 * j + jp ] = __builtin_amdgcn_mfma_f32_16x16x32_f16( fa[ ip >> 1 ][ ( ( ip & 1 ) << 1 ) + h ], fb[ ( jp << 1 ) + h ],
										acc16[ 2 * i0 + ip ][ 2 * j + jp ], 0, 0, 0 );
					}
					else
					{
	#pragma unroll
						for( int ks = 0; ks < 4; ks++ )
	#pragma unroll
							for( int i = 0; i < 2; i++ )
								acc[ i0 + i ][ j ] = __builtin_amdgcn_mfma_f32_32x32x16_f16( fa[ i ][ ks ], fb[ ks ], acc[ i0 + i ][ j ], 0, 0, 0 );
					}
					__builtin_amdgcn_s_setprio( 0 );
				};
				using I0 = std::integral_constant<int, 0>;
				using I1 = std::integral_constant<int, 1>;
				using I2 = std::integral_constant<int, 2>;

				// the tile's first operands were requested before the previous tile's epilogue (or above): K tile 0 must have landed
				if( nk > 1 )
					asm volatile( "s_waitcnt vmcnt(4)" ::: "memory" );
				else
					asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
				WH_BAR();
				if( wr == 1 ) WH_BAR();	   // wave row 1 runs one barrier behind row 0

				for( int kt = 0; kt < nk; kt++ )
				{
					const f16* const bufA = lds + ( kt & 1 ) * C::STAGE;
					const f16* const bufW = bufA + C::A_HALFS;
					const bool next = kt + 1 < nk, next2 = kt + 2 < nk;
					// phase 1: 12 fragment reads
					readB( bufW, 0, fb0 );
					readA( bufA, 0 );
					WH_BAR();
					quadrant( I0{}, I0{}, fb0 );
					WH_BAR();
					// phase 2: 4 reads, A rows 0..127 of K tile t+1
					readB( bufW, 1, fb1 );
					if( next ) stage( kt + 1, PA0{} );
					WH_BAR();
					quadrant( I0{}, I1{}, fb1 );
					WH_BAR();
					// phase 3: 8 reads, A rows 128..255 of K tile t+1
					readA( bufA, 1 );
					if( next ) stage( kt + 1, PA1{} );
					WH_BAR();
					quadrant( I2{}, I1{}, fb1 );
					WH_BAR();
					// phase 4: no reads, the W tile of K tile t+2; W and A rows 0.. of tile t+1 must have landed after the issue
					// segment, A rows 128.. after the MFMA segment
					if( next2 )
					{
						stage( kt + 2, PW0{} );
						stage( kt + 2, PW1{} );
						asm volatile( "s_waitcnt vmcnt(6)" ::: "memory" );
					}
					else if( next )
						asm volatile( "s_waitcnt vmcnt(2)" ::: "memory" );
					WH_BAR();
					quadrant( I2{}, I0{}, fb0 );
					if( next2 )
						asm volatile( "s_waitcnt vmcnt(4)" ::: "memory" );
					else
						asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
					WH_BAR();
				}
				if( wr == 0 ) WH_BAR();
				// every wave has passed the same number of barriers and retired all its fragment reads: both operand buffers are dead

				const int tmDone = tm, tnDone = tn;
				lin += linStep;
				const bool more = lin < linEnd;
				if( more )
				{
					tileCoords( lin, tm, tn );
					tileOffsets( tm, tn );
					stageFirst();	  // lands under the epilogue below
				}

				auto convert16 = [ & ]()
				{
					if constexpr( MF16 )
					{
						// 16 x 16 tiles -> the 32 x 32 register layout the general epilogues are written for (edge tiles, V tiles), one 32 x 32 block at a time through
						// the wave's 4 KiB (a wave's LDS operations execute in order: no wait between the writes, the reads and the next block's writes)
						float* const st = (float*)( smem + C::EPI_OFFSET + wave * C::EPI_PER_WAVE );
						const int q = lane >> 4, c16 = lane & 15, hi = lane >> 5, cl = lane & 31;
		#pragma unroll
						for( int i = 0; i < 4; i++ )
		#pragma unroll
							for( int j = 0; j < 2; j++ )
							{
		#pragma unroll
								for( int ti = 0; ti < 2; ti++ )
		#pragma unroll
									for( int tj = 0; tj < 2; tj++ )
		#pragma unroll
										for( int r = 0; r < 4; r++ ) st[ ( 16 * ti + 4 * q + r ) * 32 + 16 * tj + c16 ] = acc16[ 2 * i + ti ][ 2 * j + tj ][ r ];
								__builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront" );
								__builtin_amdgcn_wave_barrier();
								__builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront" );
		#pragma unroll
								for( int r = 0; r < 16; r++ ) acc[ i ][ j ][ r ] = st[ ( ( r & 3 ) + 8 * ( r >> 2 ) + 4 * hi ) * 32 + cl ];
								__builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront" );
								__builtin_amdgcn_wave_barrier();
								__builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront" );
							}

					}
				};

				bool direct = !WIDE;
				bool fastDone = false;
				if constexpr( WIDE && ( EPI == EPI_F32 || EPI == EPI_F16_GELU || EPI == EPI_QKV_ENC || EPI == EPI_CROSS_KV ) )
				{
					// interior tiles: the lean epilogue written for gemmTiled4 (no bounds checks, no divisions per row, residual rows requested a unit
					// ahead of the stores); a.wideEpi == 2 = the launcher has checked what it relies on
					const int mW = tmDone * BM + wr * 128, nW = tnDone * BN + wc * 64;
					const bool isV = EPI == EPI_QKV_ENC && nW >= 2 * a.H * HEAD_DIM;
					if( a.wideEpi == 2 && !isV && ( tmDone + 1 ) * BM <= a.M && ( tnDone + 1 ) * BN <= a.N )
					{
						unsigned char* const stage = smem + C::EPI_OFFSET + wave * C::EPI_PER_WAVE;
						if constexpr( MF16 )
						{
							if constexpr( EPI == EPI_F32 )
							{
								if( a.res )
									epilogueFast4<EPI, true, 0, 16, 2, false, true>( a, acc16, mW, nW, lane, stage );
								else
									epilogueFast4<EPI, false, 0, 16, 2, false, true>( a, acc16, mW, nW, lane, stage );
							}
							else
								epilogueFast4<EPI, false, 0, 16, 2, false, true>( a, acc16, mW, nW, lane, stage );
						}
						else if constexpr( EPI == EPI_F32 )
						{
							if( a.res )
								epilogueFast4<EPI, true, 0, 16, 2, false>( a, acc, mW, nW, lane, stage );
							else
								epilogueFast4<EPI, false, 0, 16, 2, false>( a, acc, mW, nW, lane, stage );
						}
						else
							epilogueFast4<EPI, false, 0, 16, 2, false>( a, acc, mW, nW, lane, stage );
						fastDone = true;
					}
				}
				if constexpr( MF16 )
				{
					if( !fastDone ) convert16();
				}
				if( fastDone )
				{
				}
				else
				if constexpr( WIDE && EPI == EPI_QKV_ENC )
				{
					// fragment-major V: straight from the registers (groups of 4 consecutive keys; T % 4 != 0 keeps the element-wise path)
					if( ( tnDone * BN + wc * 64 ) >= 2 * a.H * HEAD_DIM )
					{
						direct = ( a.T & 3 ) != 0;
						if( !direct )
						{
	#pragma unroll
							for( int i = 0; i < 4; i++ )
								epilogueBlockV32x64( a, acc[ i ][ 0 ], acc[ i ][ 1 ], tmDone * BM + wr * 128 + i * 32, tnDone * BN + wc * 64, lane );
						}
					}
				}
				if( fastDone )
				{
				}
				else if( direct )
					tileEpilogue<EPI, Cfg8>( a, acc, tmDone, tnDone, wr, wc, lane );
				else if( !( WIDE && EPI == EPI_QKV_ENC && ( tnDone * BN + wc * 64 ) >= 2 * a.H * HEAD_DIM ) )
				{
					if constexpr( WIDE && ( EPI == EPI_F32 || EPI == EPI_F16_GELU || EPI == EPI_CONV2 || EPI == EPI_QKV_ENC || EPI == EPI_CROSS_KV ) )
					{
#pragma unroll
						for( int i = 0; i < 4; i++ )
							epilogueBlock32x64<EPI>( a, acc[ i ][ 0 ], acc[ i ][ 1 ], tmDone * BM + wr * 128 + i * 32, tnDone * BN + wc * 64, lane,
								smem + C::EPI_OFFSET + wave * C::EPI_PER_WAVE );
					}
				}
				if( !more ) break;
			}
		}

		// ---------------------------------------------------------------------------------------------------------------
		// gemmTiled4 (round 4): the encoder product with ONE wave per SIMD -- the tile shape of the vendor library's kernel for these
		// shapes (profiles/r04_gemm_counters.txt). gemmTiled8's waves own 128 x 64 outputs, so every fragment read feeds half the MFMAs
		// it could (24 ds_read_b128 per 32 MFMAs). Here FOUR waves (2 x 2) own 128 x 128 each = 4 x 4 tiles of
		// v_mfma_f32_32x32x16_f16: 256 accumulator registers (the AGPR half of a 512-register wave), 8 fragment reads per 16 MFMAs,
		// half the LDS traffic per FLOP. With a single wave per SIMD nothing overlaps by itself, so the K loop is a software pipeline
		// written out by hand:
		//   * a K tile (64) is four substeps of 16 MFMAs in chunks of 4 (one A row tile x the four W tiles); the fragments of substep
		//     s + 1 are read (8 x ds_read_b128, second register set) behind the first 8 MFMAs of substep s, one read per MFMA
		//     (sched_group_barrier), and nothing crosses a chunk boundary (sched_barrier);
		//   * ONE s_barrier per K tile, before the LAST substep: by then a wave has read everything it needs from the current
		//     buffer (the last substep's fragments are in registers) and waited for its own LDS-DMA pieces of the next tile
		//     (vmcnt), so after the barrier the next K tile is complete in the other buffer and the current buffer is dead:
		//     the first fragments of the next K tile are read under the last substep's MFMAs and the DMA of the tile after
		//     next starts into the dead buffer, one pair of 1 KiB pieces behind each chunk of substeps 3 and 0. A piece has a whole
		//     K tile (~2k cycles) to land; the matrix pipe sees the barrier only as the skew between four waves that run the same stream;
		//   * the stream of K tiles is FLAT across output tiles (persistent workgroup, the band walk of gemmTiled8): the
		//     producer side (tile coordinates, per-lane source offsets, recomputed without a branch or a division per row) runs two
		//     K tiles ahead of the consumer and simply moves on to the next output tile; the epilogue of a tile runs between two K
		//     tiles with the next output tile's first two K tiles requested before its first store;
		//   * a tile's first substep multiplies into the constant 0 instead of clearing 256 registers;
		//   * ONE instance of every K tile position (first / middle / last) in a row and the epilogue outside the K loop: accumulators
		//     that meet at the end of alternative paths (a switch, a peeled variant) are 256 registers the allocator copies around.
		// LDS: two 64 KiB K-tile buffers (A rows, then W rows, 128-byte rows, 16-byte chunks XOR-swizzled exactly as gemmTiled8)
		// + 4 KiB of epilogue staging per wave = 144 KiB. Wave w stages rows 64 w .. 64 w + 63 of both operand tiles.
		//
		// MEASURED (MI355X, profiles/r04_gemm4_probe.txt): correct (bit-identical to gemmTiled8) and +7 .. 15 % on the plain FP32 probe
		// (168000 x 4096 x 1024: 930 against 850 TFLOP/s), but inside the model it is level with gemmTiled8 (GEMM class -2 % .. +0.3 %:
		// Q/K/V -5 %, GELU and cross-K/V +4 .. 5 %), so TUNE_GEMM_4WAVE is OFF. What it did settle, by ablation: without LDS-DMA and
		// without epilogue the K loop runs at 1500 TFLOP/s; the DMA costs 18 % of that whatever its placement (staggered over the waves,
		// spread over 2 or 3 substeps: the same) -- it is the CU's L2 -> LDS path, ~19 bytes per cycle under the MFMAs (26 alone), and a
		// 256 x 256 x 64 tile needs 64 KiB per 2048 matrix-pipe cycles = 32; the epilogue costs another 25 %: 2.5 us of instructions and
		// 4 .. 7 us in which the tile's 128 .. 256 KiB drain at the ~16 bytes per cycle a CU stores, with the next tile's DMA queued
		// behind them. Its lean epilogue, which does not depend on the wave shape, is what gemmTiled8 now uses (TUNE_GEMM_FAST_EPI).
		// An accumulator register of gemmTiled4 read where the epilogue uses it. Written as assembly so that the register allocator keeps
		// the 256 accumulators in the AGPR half of the file until then: left to itself it copies half of them into VGPRs at the end of
		// the K loop, spills the K loop's own state to scratch to make room, and every scratch reload then waits for ALL stores in
		// flight (vmcnt(0)). The MFMAs that wrote the accumulators are dozens of instructions behind the first read (the caller
		// computes the next tile's offsets in between and pads with s_nop): no hazard the compiler would have had to see.
		__device__ __forceinline__ f32x16 accReadTile( const f32x16& t )
		{
			f32x16 v;
	#pragma unroll
			for( int r = 0; r < 16; r++ )
			{
				float x;
				asm volatile( "v_accvgpr_read_b32 %0, %1" : "=v"( x ) : "a"( t[ r ] ) );
				v[ r ] = x;
			}
			return v;
		}

		// Epilogue of an INTERIOR 128 x 128 wave tile of gemmTiled4 (whole tile inside M x N; the launcher has checked what a.wideEpi == 2
		// promises below). One wave per SIMD: nothing hides a stall, so this path has no bounds checks, no divisions per row, no
		// branches, and an order of memory operations that never waits for a store:
		//   * the tile leaves in UNITS of 32 rows x 128 bytes (FP32: one MFMA tile; FP16: two side by side) through 4 KiB of LDS per
		//     wave: 16 / 32 column-wise writes per lane, then 4 x (ds_read_b128 -> 16-byte row store), 8 lanes per 128-byte row;
		//     LDS operations of a wave execute in order, so one buffer is enough and nothing but the data dependence is waited for;
		//   * software pipeline over the units, in program order: reads of unit k issued | residual rows of unit k + 1 requested |
		//     unit k + 1 converted and written to LDS (the GELU arithmetic sits here, under the LDS round trip of unit k) | unit k
		//     stored. A residual load is always older than the stores issued after it: waiting for it never waits for a store;
		//   * addresses are a scalar base per unit + one 32-bit offset per lane and row (16 registers for the 16 rows a lane stores,
		//     computed once per tile); a row past the end of its segment (sequence / conv batch) adds one constant: the wave's 128
		//     rows cross at most one boundary (segments are at least 128 rows long).
		// Same arithmetic per element as tileEpilogue / epilogueBlock32x64 (bit-identical outputs).
		// TJ = MFMA tiles per wave in N: 4 (gemmTiled4: 128 x 128 per wave) or 2 (gemmTiled8: 128 x 64); AGPR = the accumulators are read as assembly (gemmTiled4)
		// L16 (round 6): acc is f32x4[ 8 ][ 2 TJ ], the tiles of v_mfma_f32_16x16x32_f16 (lane l: column l & 15, rows 4 (l >> 4) .. + 3 of a 16 x 16 tile). Only the
		// column-wise writes into the staging area differ: a unit is the same 32 rows x 128 bytes, everything behind the LDS round trip is shared. The four row
		// groups of a tile (l >> 4) would meet in the same banks, so the 16-byte chunk index is XORed with a function of the row on both sides of the round trip.
		template<int EPI, bool HASRES, int FIRST, int LAST, int TJ, bool AGPR, bool L16, typename ACC>
		__device__ __forceinline__ void epilogueFast4( const GemmArgs& a, ACC& acc, int mW, int nW, int lane, unsigned char* stage )
		{
			static_assert( EPI == EPI_F32 || EPI == EPI_F16_GELU || EPI == EPI_QKV_ENC || EPI == EPI_CROSS_KV, "fast epilogue" );
			constexpr bool F32OUT = EPI == EPI_F32;
			constexpr bool HEADS = EPI == EPI_QKV_ENC || EPI == EPI_CROSS_KV;
			constexpr int UNITS = F32OUT ? 4 * TJ : 2 * TJ;
			constexpr int JP = TJ / 2;
			// (opaque copy: what follows is a few VALU instructions per tile; hoisted out of the tile loop it would live in scratch)
			asm volatile( "" : "+v"( lane ) );
			const int hi = lane >> 5, cl = lane & 31, rl = lane >> 3, ch = lane & 7;
			const int q16 = lane >> 4, c16 = lane & 15;
			float bias[ L16 ? 2 * TJ : TJ ];
			if constexpr( L16 )
			{
	#pragma unroll
				for( int j = 0; j < 2 * TJ; j++ ) bias[ j ] = a.bias ? a.bias[ nW + 16 * j + c16 ] : 0.0f;
			}
			else
			{
	#pragma unroll
				for( int j = 0; j < TJ; j++ ) bias[ j ] = a.bias ? a.bias[ nW + 32 * j + cl ] : 0.0f;
			}

			// ---- rows (wave-uniform): segment length, position of the tile's first row in its segment, byte offset of that row
			int seg, segPos;
			unsigned rowBytes, crossBytes;
			long long firstRowBytes;
			if constexpr( HEADS )
			{
				seg = a.T;
				const int b = mW / a.T;
				segPos = mW - b * a.T;
				rowBytes = 128u;
				crossBytes = (unsigned)( a.H - 1 ) * (unsigned)a.T * 128u;
				firstRowBytes = ( (long long)b * a.H * a.T + segPos ) * 128;
			}
			else
			{
				constexpr int ES = F32OUT ? 4 : 2;
				const int b = a.Mb > 0 ? mW / a.Mb : 0;
				seg = a.Mb > 0 ? a.Mb : 0x7fffffff;
				segPos = mW - b * ( a.Mb > 0 ? a.Mb : 0 );
				rowBytes = (unsigned)a.ldc * ES;
				crossBytes = (unsigned)( ( a.cBatchStride - (long long)a.Mb * a.ldc ) * ES );
				firstRowBytes = ( (long long)b * a.cBatchStride + (long long)segPos * a.ldc ) * ES;
			}
			seg = __builtin_amdgcn_readfirstlane( seg );
			segPos = __builtin_amdgcn_readfirstlane( segPos );
			rowBytes = __builtin_amdgcn_readfirstlane( rowBytes );
			crossBytes = __builtin_amdgcn_readfirstlane( crossBytes );
			unsigned voff[ 4 ][ 4 ];
	#pragma unroll
			for( int i = 0; i < 4; i++ )
	#pragma unroll
				for( int it = 0; it < 4; it++ )
				{
					const int r = 32 * i + 8 * it + rl;
					voff[ i ][ it ] = (unsigned)r * rowBytes + ( segPos + r >= seg ? crossBytes : 0u ) + (unsigned)ch * 16u;
				}

			// ---- columns (wave-uniform): what the wave's 128 columns are, base address of unit k
			int sel = 0;
			long long colBytes = 0;	   // byte offset of the wave tile's first column block
			if constexpr( EPI == EPI_F32 ) colBytes = (long long)nW * 4;
			if constexpr( EPI == EPI_F16_GELU ) colBytes = (long long)nW * 2;
			if constexpr( EPI == EPI_QKV_ENC )
			{
				const int d = a.H * HEAD_DIM;
				sel = __builtin_amdgcn_readfirstlane( nW / d );
				colBytes = (long long)( ( nW - sel * d ) >> 6 ) * a.T * 128;
			}
			if constexpr( EPI == EPI_CROSS_KV )
			{
				const int d = a.H * HEAD_DIM;
				const int layer = __builtin_amdgcn_readfirstlane( nW / ( 2 * d ) );
				const int c2 = nW - layer * 2 * d;
				sel = c2 >= d ? 1 : 0;
				colBytes = ( (long long)layer * a.B * a.H + ( ( sel ? c2 - d : c2 ) >> 6 ) ) * a.T * 128;
			}
			unsigned char* outBase;
			if constexpr( EPI == EPI_F32 ) outBase = (unsigned char*)a.out32;
			if constexpr( EPI == EPI_F16_GELU ) outBase = (unsigned char*)a.out16;
			if constexpr( EPI == EPI_QKV_ENC ) outBase = (unsigned char*)( sel == 0 ? a.q : a.k );
			if constexpr( EPI == EPI_CROSS_KV ) outBase = (unsigned char*)( sel ? a.v : a.k );
			outBase += firstRowBytes + colBytes;
			const unsigned char* resBase = HASRES ? (const unsigned char*)a.res + firstRowBytes + colBytes : nullptr;
			// bytes from the wave tile's first unit to unit k: FP32 unit k = MFMA tile (k / TJ, k % TJ); FP16 unit k = tiles (k / JP, 2 (k % JP)), (.., + 1)
			const long long headBytes = HEADS ? (long long)a.T * 128 : 128;

			auto writeUnit = [ & ]( auto kc )
			{
				constexpr int k = decltype( kc )::value;
				if constexpr( L16 )
				{
					// row R = 16 ti + 4 q + r of the unit; its chunk index is XORed with swz( R ) = ((R >> 2) & 1) << 2 (FP32: eight 4-column chunks per row) or
					// ((R >> 2) & 3) << 1 (FP16: eight 8-column chunks); (R >> 2) & 3 = q for every ti and r
					if constexpr( F32OUT )
					{
						constexpr int i = k / TJ, j = k % TJ;
						const int sw = ( q16 & 1 ) << 2;
	#pragma unroll
						for( int ti = 0; ti < 2; ti++ )
	#pragma unroll
							for( int tj = 0; tj < 2; tj++ )
	#pragma unroll
								for( int r = 0; r < 4; r++ )
								{
									const int row = 16 * ti + 4 * q16 + r;
									const int chunk = ( 4 * tj + ( c16 >> 2 ) ) ^ sw;
									*(float*)( stage + row * 128 + chunk * 16 + ( c16 & 3 ) * 4 ) = acc[ 2 * i + ti ][ 2 * j + tj ][ r ] + bias[ 2 * j + tj ];
								}
					}
					else
					{
						constexpr int i = k / JP, jp = k % JP;
						const int sw = q16 << 1;
	#pragma unroll
						for( int ti = 0; ti < 2; ti++ )
	#pragma unroll
							for( int tj = 0; tj < 4; tj++ )
	#pragma unroll
								for( int r = 0; r < 4; r++ )
								{
									const int row = 16 * ti + 4 * q16 + r;
									const int chunk = ( 2 * tj + ( c16 >> 3 ) ) ^ sw;
									const float v = acc[ 2 * i + ti ][ 4 * jp + tj ][ r ];
									const float b = bias[ 4 * jp + tj ];
									f16 hv;
									if constexpr( EPI == EPI_F16_GELU )
										hv = gelu16( v + b );
									else if constexpr( EPI == EPI_QKV_ENC )
										hv = (f16)( v + b );
									else
										hv = sel ? (f16)( v + b ) : (f16)( v * a.scale );
									*(f16*)( stage + row * 128 + chunk * 16 + ( c16 & 7 ) * 2 ) = hv;
								}
					}
				}
				else if constexpr( F32OUT )
				{
					constexpr int i = k / TJ, j = k % TJ;
	#pragma unroll
					for( int r = 0; r < 16; r++ )
					{
						const int row = ( r & 3 ) + 8 * ( r >> 2 ) + 4 * hi;
						float x;
						if constexpr( AGPR )
							asm volatile( "v_accvgpr_read_b32 %0, %1" : "=v"( x ) : "a"( acc[ i ][ j ][ r ] ) );
						else
							x = acc[ i ][ j ][ r ];
						*(float*)( stage + row * 128 + cl * 4 ) = x + bias[ j ];
					}
				}
				else
				{
					constexpr int i = k / JP, jp = k % JP;
	#pragma unroll
					for( int jj = 0; jj < 2; jj++ )
	#pragma unroll
						for( int r = 0; r < 16; r++ )
						{
							const int row = ( r & 3 ) + 8 * ( r >> 2 ) + 4 * hi;
							float v;
							if constexpr( AGPR )
								asm volatile( "v_accvgpr_read_b32 %0, %1" : "=v"( v ) : "a"( acc[ i ][ 2 * jp + jj ][ r ] ) );
							else
								v = acc[ i ][ 2 * jp + jj ][ r ];
							f16 hv;
							if constexpr( EPI == EPI_F16_GELU )
								hv = gelu16( v + bias[ 2 * jp + jj ] );
							else if constexpr( EPI == EPI_QKV_ENC )
								hv = (f16)( v + bias[ 2 * jp + jj ] );
							else
								hv = sel ? (f16)( v + bias[ 2 * jp + jj ] ) : (f16)( v * a.scale );
							*(f16*)( stage + row * 128 + ( jj * 32 + cl ) * 2 ) = hv;
						}
				}
			};
			auto ldsFence = [ & ]()
			{
				// compile-time only: the column-wise writes and the row-wise reads of the staging area use different types
				__builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront" );
				__builtin_amdgcn_wave_barrier();
				__builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront" );
			};
			auto unitBytes = [ & ]( int k ) -> long long { return F32OUT ? (long long)( k % TJ ) * 128 : (long long)( k % JP ) * headBytes; };
			auto loadRes = [ & ]( auto kc, f32x4( &ex )[ 4 ] )
			{
				constexpr int k = decltype( kc )::value;
				if constexpr( HASRES )
				{
					constexpr int i = F32OUT ? k / TJ : k / JP;
					const unsigned char* const b = resBase + unitBytes( k );
	#pragma unroll
					for( int it = 0; it < 4; it++ ) ex[ it ] = *(const f32x4*)( b + voff[ i ][ it ] );
				}
			};
			auto readUnit = [ & ]( f32x4( &dv )[ 4 ] )
			{
	#pragma unroll
				for( int it = 0; it < 4; it++ )
				{
					int chunk = ch;
					if constexpr( L16 )
					{
						const int row = it * 8 + rl;
						chunk = F32OUT ? ( ch ^ ( ( ( row >> 2 ) & 1 ) << 2 ) ) : ( ch ^ ( ( ( row >> 2 ) & 3 ) << 1 ) );
					}
					dv[ it ] = *(const f32x4*)( stage + ( it * 8 + rl ) * 128 + chunk * 16 );
				}
			};
			auto storeUnit = [ & ]( auto kc, const f32x4( &dv )[ 4 ], const f32x4( &ex )[ 4 ] )
			{
				constexpr int k = decltype( kc )::value;
				constexpr int i = F32OUT ? k / TJ : k / JP;
				unsigned char* const b = outBase + unitBytes( k );
	#pragma unroll
				for( int it = 0; it < 4; it++ )
				{
					f32x4 o = dv[ it ];
					if constexpr( HASRES )
					{
	#pragma unroll
						for( int e = 0; e < 4; e++ ) o[ e ] = dv[ it ][ e ] + ex[ it ][ e ];
					}
					*(f32x4*)( b + voff[ i ][ it ] ) = o;
				}
			};

			// units FIRST .. min( LAST, UNITS ) - 1 (gemmTiled4 keeps the rest of an FP16 tile in registers and stores it under the next tile's K loop)
			constexpr int U0 = FIRST, U1 = LAST < UNITS ? LAST : UNITS;
			if constexpr( U0 < U1 )
			{
				f32x4 ex[ 2 ][ 4 ], dv[ 4 ];
				loadRes( std::integral_constant<int, U0>{}, ex[ U0 & 1 ] );
				writeUnit( std::integral_constant<int, U0>{} );
				ldsFence();
				__builtin_amdgcn_sched_barrier( 0 );
				auto step = [ & ]( auto kc )
				{
					constexpr int k = decltype( kc )::value;
					if constexpr( k >= U0 && k < U1 )
					{
						readUnit( dv );
						ldsFence();
						__builtin_amdgcn_sched_barrier( 0 );
						if constexpr( k + 1 < U1 )
						{
							loadRes( std::integral_constant<int, k + 1>{}, ex[ ( k + 1 ) & 1 ] );
							writeUnit( std::integral_constant<int, k + 1>{} );
							ldsFence();
							__builtin_amdgcn_sched_barrier( 0 );
						}
						storeUnit( kc, dv, ex[ k & 1 ] );
						__builtin_amdgcn_sched_barrier( 0 );
					}
				};
				step( std::integral_constant<int, 0>{} );
				step( std::integral_constant<int, 1>{} );
				step( std::integral_constant<int, 2>{} );
				step( std::integral_constant<int, 3>{} );
				step( std::integral_constant<int, 4>{} );
				step( std::integral_constant<int, 5>{} );
				step( std::integral_constant<int, 6>{} );
				step( std::integral_constant<int, 7>{} );
				step( std::integral_constant<int, 8>{} );
				step( std::integral_constant<int, 9>{} );
				step( std::integral_constant<int, 10>{} );
				step( std::integral_constant<int, 11>{} );
				step( std::integral_constant<int, 12>{} );
				step( std::integral_constant<int, 13>{} );
				step( std::integral_constant<int, 14>{} );
				step( std::integral_constant<int, 15>{} );
			}
		}

		// The V third of the encoder's Q/K/V product, interior wave tile of gemmTiled4: fragment-major V (vFragIndex) straight from the
		// accumulators, no LDS. A lane of a 32x32 accumulator tile holds one dimension and, per register group g, the 4 consecutive keys
		// t .. t + 3 (t % 4 == 0: T % 4 == 0, launcher) -- one 8-byte half of a 16-byte fragment; the other half (keys t + 8 ..) is the
		// lane's group g + 1 or g - 1 and follows within a few instructions, so the L2 sees whole lines. Per lane 16 offsets (4 row tiles x 4 groups),
		// computed once per tile; the dimension block (+ 1 KiB) is an immediate, the head a scalar base. Same values as epilogueBlockV32x64.
		__device__ __forceinline__ void epilogueFastV4( const GemmArgs& a, f32x16 ( &acc )[ 4 ][ 4 ], int mW, int nW, int lane )
		{
			asm volatile( "" : "+v"( lane ) );
			const int hi = lane >> 5, cl = lane & 31;
			const int d = a.H * HEAD_DIM;
			float bias[ 4 ];
	#pragma unroll
			for( int j = 0; j < 4; j++ ) bias[ j ] = a.bias ? a.bias[ nW + 32 * j + cl ] : 0.0f;
			const int b = __builtin_amdgcn_readfirstlane( mW / a.T );
			const int segPos = mW - b * a.T;
			const unsigned headBytes = (unsigned)HEAD_DIM * (unsigned)a.Tpad * 2u;
			const unsigned seqBytes = (unsigned)a.H * headBytes;
			unsigned char* const base = (unsigned char*)a.v + (long long)b * seqBytes + (long long)( ( nW - 2 * d ) >> 6 ) * headBytes;
			unsigned voff[ 4 ][ 4 ];
	#pragma unroll
			for( int i = 0; i < 4; i++ )
	#pragma unroll
				for( int g = 0; g < 4; g++ )
				{
					int t = segPos + 32 * i + 8 * g + 4 * hi;
					const bool cross = t >= a.T;
					t = cross ? t - a.T : t;
					voff[ i ][ g ] = ( cross ? seqBytes : 0u ) + (unsigned)( ( ( ( t >> 4 ) * 128 + ( ( t >> 2 ) & 1 ) * 32 + cl ) * 8 + ( ( t >> 3 ) & 1 ) * 4 ) * 2 );
				}
	#pragma unroll
			for( int i = 0; i < 4; i++ )
			{
	#pragma unroll
				for( int j = 0; j < 4; j++ )
				{
					unsigned char* const bj = base + ( j >> 1 ) * (long long)headBytes + ( j & 1 ) * 1024;
	#pragma unroll
					for( int g = 0; g < 4; g++ )
					{
						f16x4 pk;
	#pragma unroll
						for( int e = 0; e < 4; e++ )
						{
							float x;
							asm volatile( "v_accvgpr_read_b32 %0, %1" : "=v"( x ) : "a"( acc[ i ][ j ][ 4 * g + e ] ) );
							pk[ e ] = (f16)( x + bias[ j ] );
						}
						*(f16x4*)( bj + voff[ i ][ g ] ) = pk;
					}
				}
				__builtin_amdgcn_sched_barrier( 0 );
			}
		}

		struct Cfg4
		{
			static constexpr int BM = 256, BN = 256, BK = 64, NT = 256, TI = 4, TJ = 4;
			static constexpr int A_BYTES = BM * BK * 2, STAGE_BYTES = ( BM + BN ) * BK * 2;	   // 32 KiB, 64 KiB
			static constexpr int EPI_OFFSET = 2 * STAGE_BYTES;
			static constexpr int EPI_PER_WAVE = 4096;
			static constexpr int LDS_BYTES = EPI_OFFSET + 4 * EPI_PER_WAVE;
		};

		// SCH (probe builds; 0 = the instance that ships; all give correct results): 1 = the DMA pieces of a K tile spread 3 / 3 / 2 over three
		// substeps (else 4 / 4 over two), 2 = the compiler's own order inside a chunk, 4 = 2 fragment reads per chunk instead of 4 + 4 + 0 + 0,
		// 16384 = no early W pieces / counted wait after the epilogue
		template<int EPI, bool WIDE, int SCH = 0>
		__global__ void __launch_bounds__( 256, 1 ) gemmTiled4( const GemmArgs a )
		{
			using C = Cfg4;
			constexpr int BM = C::BM, BN = C::BN, BK = C::BK;
			extern __shared__ __attribute__( ( aligned( 16 ) ) ) unsigned char smem[];
			typedef __attribute__( ( address_space( 3 ) ) ) void* LdsPtr;

			const int tid = threadIdx.x;
			const int lane = tid & 63;
			const int wave = __builtin_amdgcn_readfirstlane( tid >> 6 );
			const int wr = wave >> 1, wc = wave & 1;

			// ---- this workgroup's tiles (as gemmTiled8): XCD x = workgroup id % 8 owns a contiguous range of the band-walk order
			const int tilesM = ( a.M + BM - 1 ) / BM, tilesN = ( a.N + BN - 1 ) / BN;
			const int nTiles = tilesM * tilesN;
			int linFirst, linEnd, linStep;
			{
				const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
				const int q = nTiles >> 3, r = nTiles & 7;
				const int start = xcd < r ? xcd * ( q + 1 ) : r * ( q + 1 ) + ( xcd - r ) * q;
				linEnd = start + ( xcd < r ? q + 1 : q );
				linFirst = start + idx;
				linStep = ( gridDim.x + 7 - xcd ) >> 3;
			}
			auto tileCoords = [ & ]( int lin, int& tm, int& tn )
			{
				if( a.groupM > 1 )
				{
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
			};
			if( linFirst >= linEnd ) return;

			// ---- producer side: LDS-DMA sources. A tile is 32 pieces of 8 rows x 128 bytes; wave w owns pieces 8 w .. 8 w + 7 of the A
			// tile and of the W tile, issued as 4 + 4 pairs. Lane l of a piece lands at row l / 8, physical chunk l % 8, which must hold
			// logical chunk (l % 8) ^ ((row >> 1) & 7); offA / offW = byte offset of that chunk from a.A / a.W at k = 0.
			// pOff* = the output tile the producer is in (recomputed, branch-free, when it moves on to the workgroup's next tile in the middle of the consumer's K loop)
			unsigned pOffA[ 4 ][ 2 ], pOffW[ 4 ][ 2 ];
			auto tileOffsets = [ & ]( int lin, unsigned( &offA )[ 4 ][ 2 ], unsigned( &offW )[ 4 ][ 2 ] )
			{
				int tm, tn;
				tileCoords( lin, tm, tn );
				// No branch and no division per row: rows past M / N repeat the last one, a tile crosses at most one segment boundary of A
				// (segments of at least 256 rows, launcher), and everything fits 32 bits (launcher)
				const int mFirst = tm * BM, nFirst = tn * BN;
				const int mMax = a.M - 1 - mFirst, nMax = a.N - 1 - nFirst;
				int laneV = lane;
				asm volatile( "" : "+v"( laneV ) );	   // (not hoisted out of the tile loop into scratch)
				const int rIn = laneV >> 3, cPhys = laneV & 7;
				const bool segd = a.Mb > 0 && a.Mb < a.M;
				const int b0 = segd ? mFirst / a.Mb : 0;
				const int t0 = mFirst - b0 * ( segd ? a.Mb : 0 );
				const int segLeft = segd ? a.Mb - t0 : 0x7fffffff;
				const unsigned aBase = (unsigned)( ( (long long)b0 * a.aBatchStride + (long long)t0 * a.lda ) * 2 );
				const unsigned crossA = segd ? (unsigned)( ( a.aBatchStride - (long long)a.Mb * a.lda ) * 2 ) : 0u;
				const unsigned wBase = (unsigned)( (long long)nFirst * a.K * 2 );
	#pragma unroll
				for( int q = 0; q < 4; q++ )
	#pragma unroll
					for( int i = 0; i < 2; i++ )
					{
						const int row = ( wave * 8 + q * 2 + i ) * 8 + rIn;
						const unsigned c16 = (unsigned)( cPhys ^ ( ( row >> 1 ) & 7 ) ) * 16u;
						const int rm = min( row, mMax );
						offA[ q ][ i ] = aBase + (unsigned)rm * (unsigned)( a.lda * 2 ) + ( rm >= segLeft ? crossA : 0u ) + c16;
						const int rn = min( row, nMax );
						offW[ q ][ i ] = wBase + (unsigned)rn * (unsigned)( a.K * 2 ) + c16;
					}
			};
			const unsigned ldsBase = __builtin_amdgcn_readfirstlane( (unsigned)(size_t)(LdsPtr)smem );
			const unsigned pieceBase = ldsBase + (unsigned)wave * 8192u;
			const int nk = a.K / BK;	  // >= 2 (launcher)
			int pKt = 0, pLin = linFirst;
			unsigned pBufOff = 0;	  // byte offset of the buffer the producer's K tile goes to
			auto dmaA = [ & ]( auto qc )
			{
				constexpr int q = decltype( qc )::value;
				ldsDmaPair( a.A + pKt * BK, pOffA[ q ][ 0 ], pOffA[ q ][ 1 ], pieceBase + pBufOff + q * 2048 );
			};
			auto dmaW = [ & ]( auto qc )
			{
				constexpr int q = decltype( qc )::value;
				ldsDmaPair( a.W + pKt * BK, pOffW[ q ][ 0 ], pOffW[ q ][ 1 ], pieceBase + pBufOff + C::A_BYTES + q * 2048 );
			};
			using Q0 = std::integral_constant<int, 0>;
			using Q1 = std::integral_constant<int, 1>;
			using Q2 = std::integral_constant<int, 2>;
			using Q3 = std::integral_constant<int, 3>;
			// the producer's next K tile: the one after in this output tile, or K tile 0 of the workgroup's next output tile. Past the
			// workgroup's last tile it keeps issuing (valid addresses of an earlier tile, buffers nobody reads): no branch in the K loop
			auto advanceProducer = [ & ]( unsigned bufOff )
			{
				pBufOff = bufOff;
				if( ++pKt < nk ) return;
				pKt = 0;
				pLin += linStep;
				if( pLin < linEnd ) tileOffsets( pLin, pOffA, pOffW );
			};
			// Which of a K tile's 8 pairs (0..3 = A, 4..7 = W; A first: its rows are the ones that may come from HBM) goes out after chunk c
			// of substep s (s = 3: the last substep of K tile g - 2, s = 0 / 1: the first two of g - 1); -1 = none
			// pos: 0 = a K tile in the middle of an output tile, 1 = the FIRST one (its W pieces went out before the epilogue: nothing in substep 0),
			// 2 = the LAST one (substep 3 issues the next K tile's A AND W pieces: everything the first barrier after the epilogue waits for is then older
			// than the epilogue's stores, and the wait can leave those in flight)
			auto dmaAfter = [ & ]( auto sc, auto cc, auto posc )
			{
				constexpr int s = decltype( sc )::value, c = decltype( cc )::value, pos = decltype( posc )::value;
				if constexpr( ( SCH & 1 ) == 0 && ( SCH & 16384 ) == 0 )
				{
					if constexpr( pos == 1 && s == 0 ) return;
					if constexpr( pos == 2 && s == 3 )
					{
						dmaA( cc );
						dmaW( cc );
						return;
					}
				}
				constexpr int pair = ( SCH & 1 ) == 0 ? ( s == 3 ? c : s == 0 ? 4 + c : -1 )
													  : ( s == 3 ? ( c < 3 ? c : -1 ) : s == 0 ? ( c < 3 ? 3 + c : -1 ) : s == 1 ? ( c < 2 ? 6 + c : -1 ) : -1 );
				if constexpr( pair >= 4 )
					dmaW( std::integral_constant<int, ( pair >= 4 ? pair - 4 : 0 )>{} );
				else if constexpr( pair >= 0 )
					dmaA( std::integral_constant<int, ( pair >= 0 && pair < 4 ? pair : 0 )>{} );
			};

			// ---- consumer side: lane l reads row l & 31 of a 32-row tile, logical chunk 2 ks + (l >> 5), stored at chunk ^ ((row >> 1) & 7)
			const int x0 = ( lane >> 5 ) ^ ( ( lane >> 1 ) & 7 );
			unsigned aAddr[ 4 ], wAddr[ 4 ];	 // byte offsets inside a K-tile buffer, per k-substep
	#pragma unroll
			for( int ks = 0; ks < 4; ks++ )
			{
				const unsigned laneK = (unsigned)( ( lane & 31 ) * 128 + ( ( x0 ^ ( ks << 1 ) ) << 4 ) );
				aAddr[ ks ] = (unsigned)( wr * 128 * 128 ) + laneK;
				wAddr[ ks ] = (unsigned)( C::A_BYTES + wc * 128 * 128 ) + laneK;
			}
			f32x16 acc[ 4 ][ 4 ];
	#pragma unroll
			for( int i = 0; i < 4; i++ )
	#pragma unroll
				for( int j = 0; j < 4; j++ )
	#pragma unroll
					for( int r = 0; r < 16; r++ ) acc[ i ][ j ][ r ] = 0.0f;
			f16x8 fa[ 2 ][ 4 ], fb[ 2 ][ 4 ];
			// One substep (index s of its K tile) = four chunks of 4 MFMAs (A row tile c x the four W tiles) from register set SET; the
			// fragments of the NEXT substep (k-substep ksNext of the buffer at bufOff) go to set SET ^ 1: the W fragments with chunk 0,
			// the A fragments with chunk 1, so that every read has at least 8 MFMAs (256 matrix-pipe cycles) to come back. Nothing
			// crosses a chunk boundary (sched_barrier): a DMA pair issued there sits between two groups of MFMAs in the stream.
			auto substep = [ & ]( auto sc, auto setc, auto zeroc, auto posc, unsigned bufOff, int ksNext )
			{
				constexpr int SET = decltype( setc )::value;
				constexpr bool ZERO = decltype( zeroc )::value;
				const unsigned char* const pa = smem + bufOff + aAddr[ ksNext ];
				const unsigned char* const pw = smem + bufOff + wAddr[ ksNext ];
				auto chunk = [ & ]( auto cc )
				{
					constexpr int c = decltype( cc )::value;
					constexpr int RD = ( SCH & 4 ) ? 2 : 4;	   // reads per chunk: 4 + 4 + 0 + 0 or 2 + 2 + 2 + 2
					if constexpr( ( SCH & 4 ) == 0 )
					{
						if constexpr( c == 0 )
						{
	#pragma unroll
							for( int j = 0; j < 4; j++ ) fb[ SET ^ 1 ][ j ] = *(const f16x8*)( pw + j * 4096 );
						}
						if constexpr( c == 1 )
						{
	#pragma unroll
							for( int i = 0; i < 4; i++ ) fa[ SET ^ 1 ][ i ] = *(const f16x8*)( pa + i * 4096 );
						}
					}
					else
					{
						if constexpr( c < 2 )
						{
	#pragma unroll
							for( int j = 0; j < 2; j++ ) fb[ SET ^ 1 ][ 2 * c + j ] = *(const f16x8*)( pw + ( 2 * c + j ) * 4096 );
						}
						else
						{
	#pragma unroll
							for( int i = 0; i < 2; i++ ) fa[ SET ^ 1 ][ 2 * ( c - 2 ) + i ] = *(const f16x8*)( pa + ( 2 * ( c - 2 ) + i ) * 4096 );
						}
					}
					auto mfmaOne = [ & ]( int j )
					{
						if constexpr( ZERO )
						{
							const f32x16 z = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
							acc[ c ][ j ] = __builtin_amdgcn_mfma_f32_32x32x16_f16( fa[ SET ][ c ], fb[ SET ][ j ], z, 0, 0, 0 );
						}
						else
							acc[ c ][ j ] = __builtin_amdgcn_mfma_f32_32x32x16_f16( fa[ SET ][ c ], fb[ SET ][ j ], acc[ c ][ j ], 0, 0, 0 );
					};
	#pragma unroll
					for( int j = 0; j < 4; j++ ) mfmaOne( j );
					if constexpr( ( SCH & 2 ) == 0 && ( ( SCH & 4 ) != 0 || c < 2 ) )
					{
						// MFMA first, then a read behind each MFMA
	#pragma unroll
						for( int k = 0; k < RD; k++ )
						{
							__builtin_amdgcn_sched_group_barrier( 0x008, 1, 0 );
							__builtin_amdgcn_sched_group_barrier( 0x100, 1, 0 );
						}
						if constexpr( RD < 4 ) __builtin_amdgcn_sched_group_barrier( 0x008, 4 - RD, 0 );
					}
					__builtin_amdgcn_sched_barrier( 0 );
					dmaAfter( sc, cc, posc );
					__builtin_amdgcn_sched_barrier( 0 );
				};
				chunk( std::integral_constant<int, 0>{} );
				chunk( std::integral_constant<int, 1>{} );
				chunk( std::integral_constant<int, 2>{} );
				chunk( std::integral_constant<int, 3>{} );
			};
			using S0 = std::integral_constant<int, 0>;
			using S1 = std::integral_constant<int, 1>;
			using P0 = std::integral_constant<int, 0>;
			using P1 = std::integral_constant<int, 1>;
			using P2 = std::integral_constant<int, 2>;
			using P3 = std::integral_constant<int, 3>;
			using ZN = std::integral_constant<bool, false>;
			using ZY = std::integral_constant<bool, true>;

			unsigned char* const stage = smem + C::EPI_OFFSET + wave * C::EPI_PER_WAVE;

			unsigned bufOff = 0;
			// One K tile of the consumer; the fragments of its first substep are in register set 0. There is ONE instance of every K tile position
			// (first / middle / last) in a row, never alternatives: accumulators that meet at the end of alternative paths are 256 registers
			// the allocator then copies around.
			int postEpi = 0;	 // VMEM operations the last epilogue issued after the DMA pieces of the K tile that follows it (0 / 32 / 64: see the wait below)
			auto kTile = [ & ]( auto zeroc, auto posc )
			{
				constexpr int pos = decltype( posc )::value;
				substep( P0{}, S0{}, zeroc, posc, bufOff, 1 );
				substep( P1{}, S1{}, ZN{}, posc, bufOff, 2 );
				// substep 2; then every fragment of this buffer is in registers and this wave's pieces of the next K tile must have landed
				substep( P2{}, S0{}, ZN{}, posc, bufOff, 3 );
				if( pos == 1 && ( SCH & 16384 ) == 0 && postEpi >= 63 )
					// the first K tile after an epilogue: its successor's pieces are all OLDER than the epilogue's loads and stores (vmcnt is one
					// in-order queue), so they have landed as soon as no more than those are in flight -- the stores go on draining under this
					// K tile and the next
					asm volatile( "s_waitcnt vmcnt(63) lgkmcnt(0)" ::: "memory" );
				else if( pos == 1 && ( SCH & 16384 ) == 0 && postEpi >= 32 )
					asm volatile( "s_waitcnt vmcnt(32) lgkmcnt(0)" ::: "memory" );
				else
					asm volatile( "s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory" );
				WH_BAR();
				// substep 3: the next K tile is complete in the other buffer, this buffer is dead
				advanceProducer( bufOff );
				bufOff ^= (unsigned)C::STAGE_BYTES;
				substep( P3{}, S1{}, ZN{}, posc, bufOff, 0 );
			};

			auto epilogue = [ & ]( int tmD, int tnD, bool lastTile )
			{
				postEpi = 0;
				if constexpr( WIDE )
				{
					const int mW = tmD * BM + wr * 128, nW = tnD * BN + wc * 128;
					bool isV = false;
					if constexpr( EPI == EPI_QKV_ENC ) isV = nW >= 2 * a.H * HEAD_DIM;	   // 2 d is a multiple of 256: a tile is V or it is not
					const bool interior = a.wideEpi == 2 && ( tmD + 1 ) * BM <= a.M && ( tnD + 1 ) * BN <= a.N;
					if constexpr( EPI == EPI_QKV_ENC )
					{
						if( isV && interior )
						{
							epilogueFastV4( a, acc, mW, nW, lane );
							postEpi = 64;
							return;
						}
					}
					if( !isV && interior )
					{
						if constexpr( EPI == EPI_F32 )
						{
							if( a.res )
								epilogueFast4<EPI, true>( a, acc, mW, nW, lane, stage );
							else
								epilogueFast4<EPI, false>( a, acc, mW, nW, lane, stage );
						}
						else
							epilogueFast4<EPI, false>( a, acc, mW, nW, lane, stage );
						postEpi = EPI == EPI_F32 ? 64 : 32;
						return;
					}
					// edge tiles (and launches without the fast path's promises): the general block epilogues of gemmTiled8
					int laneS = lane;
					asm volatile( "" : "+v"( laneS ) );
	#pragma unroll
					for( int i = 0; i < 4; i++ )
	#pragma unroll
						for( int jp = 0; jp < 2; jp++ )
						{
							const int m0 = mW + i * 32, n0 = nW + jp * 64;
							if constexpr( EPI == EPI_QKV_ENC )
							{
								// fragment-major V straight from the registers (the launcher guarantees T % 4 == 0 for this instance)
								if( isV )
								{
									const f32x16 c0 = accReadTile( acc[ i ][ 2 * jp ] ), c1 = accReadTile( acc[ i ][ 2 * jp + 1 ] );
									epilogueBlockV32x64( a, c0, c1, m0, n0, laneS );
									__builtin_amdgcn_sched_barrier( 0 );
									continue;
								}
							}
							const f32x16 c0 = accReadTile( acc[ i ][ 2 * jp ] ), c1 = accReadTile( acc[ i ][ 2 * jp + 1 ] );
							epilogueBlock32x64<EPI>( a, c0, c1, m0, n0, laneS, stage );
							__builtin_amdgcn_sched_barrier( 0 );
						}
				}
				else
				{
					// element-wise stores (N % 8 != 0 and the like): a copy of the tile in VGPRs, most of it through scratch -- correct, not fast
					f32x16 cp[ 4 ][ 4 ];
	#pragma unroll
					for( int i = 0; i < 4; i++ )
	#pragma unroll
						for( int j = 0; j < 4; j++ ) cp[ i ][ j ] = accReadTile( acc[ i ][ j ] );
					tileEpilogue<EPI, Cfg4>( a, cp, tmD, tnD, wr, wc, lane );
				}
			};

			// ---- prologue: K tile 0 of the first output tile completely, then the first part of K tile 1
			int lin = linFirst;
			tileOffsets( lin, pOffA, pOffW );
			dmaA( Q0{} );
			dmaA( Q1{} );
			dmaA( Q2{} );
			dmaA( Q3{} );
			dmaW( Q0{} );
			dmaW( Q1{} );
			dmaW( Q2{} );
			dmaW( Q3{} );
			asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
			WH_BAR();
			advanceProducer( C::STAGE_BYTES );
			dmaA( Q0{} );
			dmaA( Q1{} );
			dmaA( Q2{} );
			if constexpr( ( SCH & 1 ) == 0 ) dmaA( Q3{} );
			if constexpr( ( SCH & 1 ) == 0 && ( SCH & 16384 ) == 0 )
			{
				dmaW( Q0{} );
				dmaW( Q1{} );
				dmaW( Q2{} );
				dmaW( Q3{} );
			}
	#pragma unroll
			for( int i = 0; i < 4; i++ ) fa[ 0 ][ i ] = *(const f16x8*)( smem + aAddr[ 0 ] + i * 4096 );
	#pragma unroll
			for( int j = 0; j < 4; j++ ) fb[ 0 ][ j ] = *(const f16x8*)( smem + wAddr[ 0 ] + j * 4096 );
			__builtin_amdgcn_sched_barrier( 0 );

			using KM = std::integral_constant<int, 0>;
			using KF = std::integral_constant<int, 1>;
			using KL = std::integral_constant<int, 2>;
			for( ;; )
			{
				// first, middle, last (nk >= 2)
				kTile( ZY{}, KF{} );
				for( int kt = 1; kt + 1 < nk; kt++ ) kTile( ZN{}, KM{} );
				kTile( ZN{}, KL{} );
				int tm, tn;
				tileCoords( lin, tm, tn );
				asm volatile( "s_nop 15\n\ts_nop 15" ::: "memory" );	   // the last MFMA's 16 passes are over before the first accumulator is read
				epilogue( tm, tn, lin + linStep >= linEnd );
				lin += linStep;
				if( lin >= linEnd ) break;
			}
			// the producer ran ahead: nothing of it may land after the workgroup has given its LDS back
			asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
		}
	}	// namespace

	// What epilogueFast4 relies on (interior tiles of the two persistent kernels): a wave's 128 rows cross at most one segment boundary, and
	// everything it adds per lane fits 32 bits
	template<int EPI>
	static bool fastEpilogueOk( const GemmArgs& a )
	{
		if( EPI == EPI_QKV_ENC || EPI == EPI_CROSS_KV )
			return a.T >= 128 && ( a.H * HEAD_DIM ) % 128 == 0 && (long long)( a.H - 1 ) * a.T * 128 < ( 1ll << 31 );
		if( EPI != EPI_F32 && EPI != EPI_F16_GELU ) return false;
		const int es = EPI == EPI_F32 ? 4 : 2;
		bool fast = (long long)a.ldc * es * 128 < ( 1ll << 31 );
		if( a.Mb > 0 && a.Mb < a.M )
		{
			const long long cross = ( a.cBatchStride - (long long)a.Mb * a.ldc ) * es;
			fast = fast && a.Mb >= 128 && cross >= 0 && cross + (long long)a.ldc * es * 128 < ( 1ll << 31 );
		}
		return fast;
	}

	// CUs of the calling thread's device, asked once per device (256 when the device does not say)
	static int cuCount( int& cus )
	{
		static std::atomic<int> cusOfDevice[ 64 ];
		int dev = 0;
		if( hipGetDevice( &dev ) != hipSuccess ) dev = 0;
		if( ( cus = cusOfDevice[ dev & 63 ].load( std::memory_order_relaxed ) ) > 0 ) return 0;
		WH_HIP( hipDeviceGetAttribute( &cus, hipDeviceAttributeMultiprocessorCount, dev ) );
		if( cus <= 0 ) cus = 256;
		cusOfDevice[ dev & 63 ].store( cus, std::memory_order_relaxed );
		return 0;
	}

	// WH_GEMM_GROUP_M: M tiles per band of the walk, for A/B runs (4: the band's A rows are 2 MB of an XCD's 4 MB L2 at K = 1024 and W is re-streamed once per band)
	static int defaultGroupM()
	{
		static const int groupEnv = []() { const char* e = getenv( "WH_GEMM_GROUP_M" ); const int v = e ? atoi( e ) : 0; return v >= 1 && v <= 64 ? v : 0; }();
		return groupEnv ? groupEnv : ( ( g_tuning & TUNE_GEMM_GROUP_M ) ? 4 : 1 );
	}

	// Wide / Narrow = the kernel's instances with and without the LDS-transposed epilogue, C = Cfg8 or Cfg4, WITH_V: see wideEpilogueOk
	template<int EPI, class C, auto Wide, auto Narrow, bool WITH_V>
	static int launchPersistent( const GemmArgs& a, bool fastEpi, hipStream_t stream )
	{
		GemmArgs b = a;
		if( b.groupM == 0 ) b.groupM = defaultGroupM();
		const bool wide = wideEpilogueOk( a, EPI, WITH_V );
		b.wideEpi = t_gemmWideEpi = wide ? ( fastEpi && fastEpilogueOk<EPI>( a ) ? 2 : 1 ) : 0;
		// persistent: one workgroup per CU (gemmTiled8's takes all 160 KiB of LDS, gemmTiled4's 512 registers per lane: one wave per SIMD), each walks its share of the tiles
		const int tiles = ( ( b.M + C::BM - 1 ) / C::BM ) * ( ( b.N + C::BN - 1 ) / C::BN );
		int cus = 0;
		WH_CHECK( cuCount( cus ) );
		if( b.cuLimit > 0 && b.cuLimit < cus ) cus = b.cuLimit;
		const dim3 grid( tiles < cus ? tiles : cus ), block( C::NT );
		return wide ? launchLds<Wide>( grid, block, C::LDS_BYTES, stream, b ) : launchLds<Narrow>( grid, block, C::LDS_BYTES, stream, b );
	}

	// the 8-wave kernel; interior tiles leave through gemmTiled4's epilogue under TUNE_GEMM_FAST_EPI (the V columns of the encoder's Q/K/V product with T % 4 == 0)
	template<int EPI, bool MF16>
	static int launchTiled8T( const GemmArgs& a, hipStream_t stream )
	{
		const bool fastEpi = ( g_tuning & TUNE_GEMM_FAST_EPI ) && ( EPI != EPI_QKV_ENC || ( a.T % 4 ) == 0 );
		return launchPersistent<EPI, Cfg8, gemmTiled8<EPI, true, MF16>, gemmTiled8<EPI, false, MF16>, false>( a, fastEpi, stream );
	}
	// the 4-wave kernel; its wide epilogue takes the V columns too
	template<int EPI, int SCH = 0>
	static int launchTiled4T( const GemmArgs& a, hipStream_t stream )
	{
		return launchPersistent<EPI, Cfg4, gemmTiled4<EPI, true, SCH>, gemmTiled4<EPI, false, SCH>, true>( a, true, stream );
	}

	bool persistentEpilogue( int epi ) { return epi == EPI_F32 || epi == EPI_F16_GELU || epi == EPI_QKV_ENC || epi == EPI_CROSS_KV; }

	int launchTiled8( const GemmArgs& a, bool mf16, hipStream_t stream )
	{
		switch( a.epi )
		{
		case EPI_F32: return mf16 ? launchTiled8T<EPI_F32, true>( a, stream ) : launchTiled8T<EPI_F32, false>( a, stream );
		case EPI_F16_GELU: return mf16 ? launchTiled8T<EPI_F16_GELU, true>( a, stream ) : launchTiled8T<EPI_F16_GELU, false>( a, stream );
		case EPI_QKV_ENC: return mf16 ? launchTiled8T<EPI_QKV_ENC, true>( a, stream ) : launchTiled8T<EPI_QKV_ENC, false>( a, stream );
		case EPI_CROSS_KV: return mf16 ? launchTiled8T<EPI_CROSS_KV, true>( a, stream ) : launchTiled8T<EPI_CROSS_KV, false>( a, stream );
		}
		setError( "gemm: epilogue not available in the persistent kernels" );
		return -1;
	}

	int launchTiled4( const GemmArgs& a, hipStream_t stream )
	{
		switch( a.epi )
		{
		case EPI_F32: return launchTiled4T<EPI_F32>( a, stream );
		case EPI_F16_GELU: return launchTiled4T<EPI_F16_GELU>( a, stream );
		case EPI_QKV_ENC: return launchTiled4T<EPI_QKV_ENC>( a, stream );
		case EPI_CROSS_KV: return launchTiled4T<EPI_CROSS_KV>( a, stream );
		}
		setError( "gemm: epilogue not available in the persistent kernels" );
		return -1;
	}
#ifdef WH_PROBES
	int launchTiled4Probe( const GemmArgs& a, hipStream_t stream ) { return launchTiled4T<EPI_F32, 16384>( a, stream ); }
#endif
}
