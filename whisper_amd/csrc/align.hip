// Token alignment (word-level timestamps): cross-attention weights of chosen decoder heads -> softmax -> column standardisation -> median of 7 ->
// mean over the heads -> dynamic time warping. The definition is DESIGN.md "Token alignment" (restated in numpy by tests/align_ref.py); the kernels keep
// next to the entry points that own their buffers, like resample.hip and vad.hip.
//
//   alignStats   sweep 1: per (window, head, row) the maximum and the sum of exp( S - max ) over the window's keys. One wave per 16 rows; S on
//                v_mfma_f32_16x16x32_f16 (a 64-deep dot product is two instructions), the sum in FP64 in key order.
//   alignMatrix  sweep 2: a workgroup owns 26 keys of a window (a 32-key slab with the median's halo of 3 on both sides) and ALL rows. Per head, in the
//                fixed head order: S again (same instructions, same bits), P into the LDS slab, the column statistics over the rows in FP64, Z in place,
//                then thread r filters row r and adds to its 26 accumulators in registers. Per-head weights never reach memory.
//   dtw          one 256-thread workgroup per window, thread i = row i, one anti-diagonal per step; the last two diagonals in LDS, the trace packed
//                2 bits per cell in LDS (96 KB at 256 x 1500), walked back by one lane. Only the frames leave the device.
// No atomics; every sum has a fixed order that depends on the window's own rows and keys only, so the bits of M do not depend on the batch size, the
// window's place in the batch or the padding.
#include "runtime.h"

namespace wh
{
	namespace
	{
		constexpr int AL_MAX_ROWS = 256;	 // rows of a window: n_text_ctx / 2 + 4 <= 228 for every model
		constexpr int AL_SLAB = 32;			 // keys in a workgroup's slab
		constexpr int AL_HALO = 3;
		constexpr int AL_OUT = AL_SLAB - 2 * AL_HALO;	  // keys a workgroup writes
		constexpr int AL_LD = AL_SLAB + 1;	 // slab row stride in floats: thread r reads row r, ( 33 r + c ) mod 32 spreads a wave over the banks

		struct AlignArgs
		{
			const f16* q;			// [layer - qLayer0][window][nMax][H * 64]
			const f16* k;			// [layer][window][H][keyStride][64]
			long long qLayerStride, kLayerStride;
			int qLayer0, nLayers, H, keyStride;
			const int* heads;		// device [nHeads][2] = (layer, head)
			int nHeads;
			const int* rows;		// device [windows]
			const int* keys;		// device [windows]
			int windows, nMax, keyMax;
			float* stats;			// [windows][nHeads][nMax][2] = (max, sum)
			float* M;				// [windows][nMax][keyMax]
		};

		__device__ __forceinline__ int clampi( int v, int lo, int hi ) { return v < lo ? lo : ( v > hi ? hi : v ); }

		// what both sweeps need of a (window, head index): the operand bases and the window's sizes, every index clamped into the buffers
		struct HeadView { const f16* q; const f16* k; };
		__device__ __forceinline__ HeadView headView( const AlignArgs& a, int w, int hi )
		{
			const int layer = clampi( a.heads[ 2 * hi ], a.qLayer0, a.nLayers - 1 );
			const int head = clampi( a.heads[ 2 * hi + 1 ], 0, a.H - 1 );
			HeadView v;
			v.q = a.q + (long long)( layer - a.qLayer0 ) * a.qLayerStride + (long long)w * a.nMax * a.H * HEAD_DIM + head * HEAD_DIM;
			v.k = a.k + (long long)layer * a.kLayerStride + ( (long long)w * a.H + head ) * a.keyStride * HEAD_DIM;
			return v;
		}

		// S^T tile: 16 keys (operand A, key = lane & 15) x 16 rows (operand B, row = lane & 15); lane holds row lane & 15, keys 4 (lane >> 4) + r
		__device__ __forceinline__ f32x4 scoreTile( const f16x8 k0, const f16x8 k1, const f16x8 q0, const f16x8 q1 )
		{
			f32x4 s = { 0.0f, 0.0f, 0.0f, 0.0f };
			s = __builtin_amdgcn_mfma_f32_16x16x32_f16( k0, q0, s, 0, 0, 0 );
			s = __builtin_amdgcn_mfma_f32_16x16x32_f16( k1, q1, s, 0, 0, 0 );
			return s;
		}

		__global__ __launch_bounds__( 64 ) void alignStats( const AlignArgs a )
		{
			const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
			const int rt = blockIdx.x, hi = blockIdx.y, w = blockIdx.z;
			const int rows = clampi( a.rows[ w ], 0, a.nMax );
			const int keys = clampi( a.keys[ w ], 0, a.keyMax < a.keyStride ? a.keyMax : a.keyStride );
			if( rt * 16 >= rows || keys <= 0 ) return;
			const HeadView v = headView( a, w, hi );
			const int row = rt * 16 + lr;
			const int rowL = row < rows ? row : rows - 1;
			const f16* const qp = v.q + (long long)rowL * a.H * HEAD_DIM + lg * 8;
			const f16x8 q0 = *(const f16x8*)qp, q1 = *(const f16x8*)( qp + 32 );
			const int nTiles = ( keys + 15 ) >> 4;
			auto tile = [ & ]( int t ) -> f32x4
			{
				int key = t * 16 + lr;
				key = key < keys ? key : keys - 1;
				const f16* const kp = v.k + (long long)key * HEAD_DIM + lg * 8;
				return scoreTile( *(const f16x8*)kp, *(const f16x8*)( kp + 32 ), q0, q1 );
			};
			float mx = -INFINITY;
			for( int t = 0; t < nTiles; t++ )
			{
				const f32x4 s = tile( t );
#pragma unroll
				for( int r = 0; r < 4; r++ )
					if( t * 16 + lg * 4 + r < keys ) mx = fmaxf( mx, s[ r ] );
			}
			mx = fmaxf( mx, __shfl_xor( mx, 16, 64 ) );
			mx = fmaxf( mx, __shfl_xor( mx, 32, 64 ) );
			double sum = 0.0;
			for( int t = 0; t < nTiles; t++ )
			{
				const f32x4 s = tile( t );
#pragma unroll
				for( int r = 0; r < 4; r++ )
					if( t * 16 + lg * 4 + r < keys ) sum += (double)expf( s[ r ] - mx );
			}
			// the four key groups of a row, added in group order
			const double s0 = __shfl( sum, lr, 64 ), s1 = __shfl( sum, lr + 16, 64 ), s2 = __shfl( sum, lr + 32, 64 ), s3 = __shfl( sum, lr + 48, 64 );
			const double total = ( ( s0 + s1 ) + s2 ) + s3;
			if( lg == 0 && row < rows )
			{
				float* const o = a.stats + ( ( (long long)w * a.nHeads + hi ) * a.nMax + row ) * 2;
				o[ 0 ] = mx;
				o[ 1 ] = (float)total;
			}
		}

		__device__ __forceinline__ void cswap( float& x, float& y )
		{
			const float lo = fminf( x, y ), hi = fmaxf( x, y );
			x = lo; y = hi;
		}
		// the 4th of 7: a 16-exchange sorting network
		__device__ __forceinline__ float median7( float v0, float v1, float v2, float v3, float v4, float v5, float v6 )
		{
			cswap( v0, v6 ); cswap( v2, v3 ); cswap( v4, v5 );
			cswap( v0, v2 ); cswap( v1, v4 ); cswap( v3, v6 );
			cswap( v0, v1 ); cswap( v2, v5 ); cswap( v3, v4 );
			cswap( v1, v2 ); cswap( v4, v6 );
			cswap( v2, v3 ); cswap( v4, v5 );
			cswap( v1, v2 ); cswap( v3, v4 ); cswap( v5, v6 );
			return v3;
		}

		__global__ __launch_bounds__( 256 ) void alignMatrix( const AlignArgs a )
		{
			__shared__ float slab[ AL_MAX_ROWS * AL_LD ];
			__shared__ double part[ 8 ][ AL_SLAB ];
			__shared__ double colMean[ AL_SLAB ], colStd[ AL_SLAB ];

			const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
			const int kt = blockIdx.x, w = blockIdx.y;
			const int rows = clampi( a.rows[ w ], 0, a.nMax );
			const int keys = clampi( a.keys[ w ], 0, a.keyMax < a.keyStride ? a.keyMax : a.keyStride );
			const int k0 = kt * AL_OUT;			// first key this workgroup writes; slab column s is key k0 - AL_HALO + s
			float* const Mw = a.M + (long long)w * a.nMax * a.keyMax;

			float acc[ AL_OUT ];
#pragma unroll
			for( int o = 0; o < AL_OUT; o++ ) acc[ o ] = 0.0f;

			const bool live = rows > 0 && k0 < keys;
			if( live )
			{
				const int nRowTiles = ( rows + 15 ) >> 4;
				const int colT = tid & 31, partT = tid >> 5;
				for( int hi = 0; hi < a.nHeads; hi++ )
				{
					const HeadView v = headView( a, w, hi );
					const float* const st = a.stats + ( ( (long long)w * a.nHeads + hi ) * a.nMax ) * 2;
					// ---- P into the slab: the wave's row tiles x the two 16-key halves ----
					f16x8 kf[ 2 ][ 2 ];
#pragma unroll
					for( int half = 0; half < 2; half++ )
					{
						const int key = clampi( k0 - AL_HALO + half * 16 + lr, 0, keys - 1 );
						const f16* const kp = v.k + (long long)key * HEAD_DIM + lg * 8;
						kf[ half ][ 0 ] = *(const f16x8*)kp;
						kf[ half ][ 1 ] = *(const f16x8*)( kp + 32 );
					}
					for( int rt = wave; rt < nRowTiles; rt += 4 )
					{
						const int row = rt * 16 + lr;
						const int rowL = row < rows ? row : rows - 1;
						const f16* const qp = v.q + (long long)rowL * a.H * HEAD_DIM + lg * 8;
						const f16x8 q0 = *(const f16x8*)qp, q1 = *(const f16x8*)( qp + 32 );
						const float mx = st[ 2 * rowL ], sum = st[ 2 * rowL + 1 ];
#pragma unroll
						for( int half = 0; half < 2; half++ )
						{
							const f32x4 s = scoreTile( kf[ half ][ 0 ], kf[ half ][ 1 ], q0, q1 );
#pragma unroll
							for( int r = 0; r < 4; r++ )
							{
								const int sc = half * 16 + lg * 4 + r;
								const int key = k0 - AL_HALO + sc;
								const float p = ( key >= 0 && key < keys ) ? expf( s[ r ] - mx ) / sum : 0.0f;
								if( row < rows ) slab[ row * AL_LD + sc ] = p;
							}
						}
					}
					__syncthreads();
					// ---- column statistics over the window's rows: 8 ranges of 32 rows in row order, the ranges added in range order ----
					{
						const int r0 = partT * 32, r1 = r0 + 32 < rows ? r0 + 32 : rows;
						double s = 0.0;
						for( int r = r0; r < r1; r++ ) s += (double)slab[ r * AL_LD + colT ];
						part[ partT ][ colT ] = s;
						__syncthreads();
						double tot = part[ 0 ][ colT ];
#pragma unroll
						for( int i = 1; i < 8; i++ ) tot += part[ i ][ colT ];
						const double mean = tot / (double)rows;
						__syncthreads();
						double s2 = 0.0;
						for( int r = r0; r < r1; r++ )
						{
							const double dv = (double)slab[ r * AL_LD + colT ] - mean;
							s2 += dv * dv;
						}
						part[ partT ][ colT ] = s2;
						__syncthreads();
						if( partT == 0 )
						{
							double t2 = part[ 0 ][ colT ];
#pragma unroll
							for( int i = 1; i < 8; i++ ) t2 += part[ i ][ colT ];
							colMean[ colT ] = mean;
							colStd[ colT ] = sqrt( t2 / (double)rows );
						}
						__syncthreads();
					}
					// ---- thread r: Z of row r in place, then the median of 7 with reflect padding, added in head order ----
					if( tid < rows )
					{
						float* const rowp = slab + tid * AL_LD;
#pragma unroll
						for( int s = 0; s < AL_SLAB; s++ )
						{
							const double sd = colStd[ s ];
							rowp[ s ] = sd > 0.0 ? (float)( ( (double)rowp[ s ] - colMean[ s ] ) / sd ) : 0.0f;
						}
						if( keys <= 3 )
						{
#pragma unroll
							for( int o = 0; o < AL_OUT; o++ ) acc[ o ] += rowp[ o + AL_HALO ];
						}
						else
						{
							const int last2 = 2 * ( keys - 1 );
							auto at = [ & ]( int key ) -> float
							{
								key = key < 0 ? -key : key;
								key = key >= keys ? last2 - key : key;
								return rowp[ key - k0 + AL_HALO ];
							};
#pragma unroll
							for( int o = 0; o < AL_OUT; o++ )
							{
								const int key = k0 + o;
								if( key < keys )
									acc[ o ] += median7( at( key - 3 ), at( key - 2 ), at( key - 1 ), at( key ), at( key + 1 ), at( key + 2 ), at( key + 3 ) );
							}
						}
					}
					__syncthreads();
				}
			}
			// ---- M: the mean over the heads; zero outside the window's rows and keys ----
			const float nH = (float)a.nHeads;
			for( int row = tid; row < a.nMax; row += 256 )
#pragma unroll
				for( int o = 0; o < AL_OUT; o++ )
				{
					const int key = k0 + o;
					if( key < a.keyMax ) Mw[ (long long)row * a.keyMax + key ] = ( live && row < rows && key < keys ) ? acc[ o ] / nH : 0.0f;
				}
		}

		struct DtwArgs
		{
			const float* x;			// cost = sign * x[ window ][ rowOff + r ][ key ]
			long long windowStride;
			int rowStride, negate;
			const int* rowOff;		// device [windows] or null
			const int* R;			// device [windows]
			const int* keys;		// device [windows]
			int rowMax, keyMax;		// bounds of R and keys: they size the trace
			int* frames;			// [windows][frameStride]
			int frameStride;
		};

		__global__ __launch_bounds__( 256 ) void dtw( const DtwArgs a )
		{
			extern __shared__ unsigned int trace[];	   // [R][ wpr ] 2 bits per cell
			__shared__ float diag[ 3 ][ AL_MAX_ROWS + 1 ];
			__shared__ int frameL[ AL_MAX_ROWS ];

			const int tid = threadIdx.x, w = blockIdx.x;
			const int R = clampi( a.R[ w ], 0, a.rowMax );
			const int N = clampi( a.keys[ w ], 0, a.keyMax );
			int* const out = a.frames + (long long)w * a.frameStride;
			if( R == 0 || N == 0 )
			{
				for( int r = tid; r < a.frameStride; r += 256 ) out[ r ] = -1;
				return;
			}
			const int wpr = ( a.keyMax + 15 ) >> 4;
			const int i = tid + 1;			// this thread's row of the cost table
			const bool mineRow = i <= R;
			const int off = a.rowOff ? a.rowOff[ w ] : 0;
			const float* const xr = a.x + (long long)w * a.windowStride + (long long)( off + tid ) * a.rowStride;
			auto loadX = [ & ]( int j ) -> float
			{
				const float v = xr[ j - 1 ];
				return a.negate ? -v : v;
			};
			float left = INFINITY;			// cost[ i ][ j - 1 ]; column 0 is +inf
			float xNext = mineRow ? loadX( 1 ) : 0.0f;
			unsigned int word = 0;
			for( int d = 2; d <= R + N; d++ )
			{
				const int j = d - i;
				if( mineRow && j >= 1 && j <= N )
				{
					const float xv = xNext;
					if( j < N ) xNext = loadX( j + 1 );
					float c0, c1;
					if( i == 1 )
					{
						c0 = j == 1 ? 0.0f : INFINITY;
						c1 = INFINITY;
					}
					else
					{
						c0 = j == 1 ? INFINITY : diag[ ( d - 2 ) % 3 ][ i - 1 ];
						c1 = diag[ ( d - 1 ) % 3 ][ i - 1 ];
					}
					const float c2 = left;
					const unsigned int t = ( c0 < c1 && c0 < c2 ) ? 0u : ( ( c1 < c0 && c1 < c2 ) ? 1u : 2u );
					const float c = xv + fminf( fminf( c0, c1 ), c2 );
					left = c;
					diag[ d % 3 ][ i ] = c;
					word |= t << ( 2 * ( ( j - 1 ) & 15 ) );
					if( ( ( j - 1 ) & 15 ) == 15 || j == N )
					{
						trace[ tid * wpr + ( ( j - 1 ) >> 4 ) ] = word;
						word = 0;
					}
				}
				__syncthreads();
			}
			// ---- walk back from ( R, N ): row 0 of the table is all 2, column 0 all 1 ----
			if( tid == 0 )
			{
				int ii = R, jj = N;
				while( ii > 0 || jj > 0 )
				{
					if( ii > 0 ) frameL[ ii - 1 ] = jj > 0 ? jj - 1 : 0;	 // j only falls along the path: the last write of a row is its smallest key
					unsigned int t;
					if( ii == 0 ) t = 2;
					else if( jj == 0 ) t = 1;
					else t = ( trace[ ( ii - 1 ) * wpr + ( ( jj - 1 ) >> 4 ) ] >> ( 2 * ( ( jj - 1 ) & 15 ) ) ) & 3u;
					if( t == 0 ) { ii--; jj--; }
					else if( t == 1 ) ii--;
					else jj--;
				}
			}
			__syncthreads();
			for( int r = tid; r < a.frameStride; r += 256 ) out[ r ] = r < R ? frameL[ r ] : -1;
		}

		int launchAlignMatrix( const AlignArgs& a, hipStream_t stream )
		{
			if( !a.q || !a.k || !a.heads || !a.rows || !a.keys || !a.stats || !a.M || a.nHeads <= 0 || a.windows <= 0 || a.nMax <= 0 || a.nMax > AL_MAX_ROWS ||
				a.keyMax <= 0 || a.keyStride <= 0 || a.H <= 0 || a.nLayers <= a.qLayer0 || a.qLayer0 < 0 || a.nHeads > 65535 || a.windows > 65535 )
			{
				setError( "align_matrix: bad argument (1 .. 256 rows per window, at least one head and one key)" );
				return WH_E_INVALIDARG;
			}
			hipLaunchKernelGGL( alignStats, dim3( ( a.nMax + 15 ) / 16, a.nHeads, a.windows ), dim3( 64 ), 0, stream, a );
			WH_HIP( hipGetLastError() );
			hipLaunchKernelGGL( alignMatrix, dim3( ( a.keyMax + AL_OUT - 1 ) / AL_OUT, a.windows ), dim3( 256 ), 0, stream, a );
			WH_HIP( hipGetLastError() );
			return 0;
		}

		int launchDtw( const DtwArgs& a, int windows, hipStream_t stream )
		{
			const size_t lds = (size_t)a.rowMax * ( ( a.keyMax + 15 ) / 16 ) * 4;
			if( !a.x || !a.R || !a.keys || !a.frames || windows <= 0 || a.rowMax <= 0 || a.rowMax > AL_MAX_ROWS || a.keyMax <= 0 || a.frameStride < a.rowMax ||
				lds > 150 * 1024 )
			{
				setError( "dtw: bad argument (1 .. 256 rows, the packed trace of rows x keys within 150 KB of LDS)" );
				return WH_E_INVALIDARG;
			}
			return launchLds<dtw, 150 * 1024>( dim3( windows ), dim3( 256 ), lds, stream, a );
		}
	}	// namespace

	// "align-matrix" / "align-q" of wh_debug_read: 1 = not one of ours
	int alignDebugRead( wh_context* c, const std::string& w, int layer, float* dstHost, int64_t dstCapFloats )
	{
		if( w != "align-matrix" && w != "align-q" ) return 1;
		if( !c->alignM || c->alignBatch <= 0 ) { setError( "debug_read: wh_align_tokens has not run" ); return WH_E_NOT_READY; }
		WH_HIP( hipStreamSynchronize( c->stream ) );
		if( w == "align-matrix" )
		{
			// the last call's M, [batch][nMax][audio context]
			const int64_t n = (int64_t)c->alignBatch * c->alignNMax * c->T;
			if( dstCapFloats < n ) return WH_E_BOUNDS;
			WH_HIP( hipMemcpy( dstHost, c->alignM, (size_t)n * 4, hipMemcpyDeviceToHost ) );
			return 0;
		}
		// the cross-attention query rows of `layer` as the last call's pass formed them, [batch * nMax][d]
		if( layer < c->alignLayer0 || layer > c->alignLayer1 ) { setError( "debug_read: align-q holds the layers of the selected heads only" ); return WH_E_BOUNDS; }
		const int64_t n = (int64_t)c->alignBatch * c->alignNMax * c->m->hp.n_text_state;
		if( dstCapFloats < n ) return WH_E_BOUNDS;
		std::vector<uint16_t> tmp( (size_t)n );
		WH_HIP( hipMemcpy( tmp.data(), c->alignQ + (int64_t)( layer - c->alignLayer0 ) * n, (size_t)n * 2, hipMemcpyDeviceToHost ) );
		for( int64_t i = 0; i < n; i++ ) dstHost[ i ] = f16BitsToF32( tmp[ (size_t)i ] );
		return 0;
	}
}	// namespace wh

extern "C" {

int wh_model_set_alignment_heads( wh_model* m, const int32_t* layerHeadPairs, int count )
{
	if( !m || count < 0 || ( count > 0 && !layerHeadPairs ) ) { setError( "model_set_alignment_heads: bad argument" ); return WH_E_INVALIDARG; }
	for( int i = 0; i < count; i++ )
		if( layerHeadPairs[ 2 * i ] < 0 || layerHeadPairs[ 2 * i ] >= m->hp.n_text_layer || layerHeadPairs[ 2 * i + 1 ] < 0 || layerHeadPairs[ 2 * i + 1 ] >= m->hp.n_text_head )
		{
			setError( "model_set_alignment_heads: pair " + std::to_string( i ) + " is outside the decoder's layers and heads" );
			return WH_E_INVALIDARG;
		}
	// ascending layer, then ascending head; a pair named twice counts once
	std::set<std::pair<int32_t, int32_t>> sorted;
	for( int i = 0; i < count; i++ ) sorted.insert( { layerHeadPairs[ 2 * i ], layerHeadPairs[ 2 * i + 1 ] } );
	m->alignHeads.clear();
	for( const auto& p : sorted ) { m->alignHeads.push_back( p.first ); m->alignHeads.push_back( p.second ); }
	return 0;
}

int wh_op_align_matrix( void* stream, const void* qF16, int64_t qLayerStride, int qLayer0, const void* kCache, int64_t kLayerStride, int nLayers, int heads, int keyStride,
	const int32_t* headPairsDev, int nHeads, const int32_t* rowsDev, const int32_t* keysDev, int windows, int nMax, int keyMax, float* statsDev, float* mDev )
{
	AlignArgs a = {};
	a.q = (const f16*)qF16; a.k = (const f16*)kCache; a.qLayerStride = qLayerStride; a.kLayerStride = kLayerStride;
	a.qLayer0 = qLayer0; a.nLayers = nLayers; a.H = heads; a.keyStride = keyStride;
	a.heads = headPairsDev; a.nHeads = nHeads; a.rows = rowsDev; a.keys = keysDev;
	a.windows = windows; a.nMax = nMax; a.keyMax = keyMax; a.stats = statsDev; a.M = mDev;
	return launchAlignMatrix( a, (hipStream_t)stream );
}

int wh_op_dtw( void* stream, const float* xDev, int windows, int rowMax, int keyMax, const int32_t* rowsDev, const int32_t* keysDev, int32_t* framesDev )
{
	DtwArgs a = {};
	a.x = xDev; a.windowStride = (long long)rowMax * keyMax; a.rowStride = keyMax; a.negate = 0; a.rowOff = nullptr;
	a.R = rowsDev; a.keys = keysDev; a.rowMax = rowMax; a.keyMax = keyMax; a.frames = framesDev; a.frameStride = rowMax;
	return launchDtw( a, windows, (hipStream_t)stream );
}

int wh_align_tokens( wh_context* c, int batch, const int32_t* tokens, const int32_t* lens, const int32_t* nKeys, int nMax, int32_t* framesHost )
{
	if( !c || !tokens || !lens || !nKeys || !framesHost || batch <= 0 || nMax <= 0 ) { setError( "align_tokens: bad argument" ); return WH_E_INVALIDARG; }
	if( c->hyp != 1 ) { setError( "align_tokens: greedy contexts only (one hypothesis per window)" ); return WH_E_INVALIDARG; }
	if( c->flags & WH_FLAG_PARITY_EXACT ) { setError( "align_tokens: not under WH_FLAG_PARITY_EXACT" ); return WH_E_INVALIDARG; }
	if( !c->encoded ) { setError( "align_tokens: wh_encode has not run" ); return WH_E_NOT_READY; }
	if( batch > c->lastEncBatch ) { setError( "align_tokens: more windows than the last wh_encode filled" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	const wh_model* m = c->m;
	const wh_hparams& hp = m->hp;
	const int d = hp.n_text_state;
	if( nMax > AL_MAX_ROWS || nMax > hp.n_text_ctx || (int64_t)batch * nMax > c->pinTokenCap() ) { setError( "align_tokens: too many tokens per window" ); return WH_E_BOUNDS; }
	const int tnot = specialIds( hp ).tnot;
	// per window: the rows fed, where the text begins (behind the first no-timestamps token), the rows of the cost matrix
	std::vector<int32_t> heads = m->alignHeads;
	if( heads.empty() )
		for( int l = hp.n_text_layer / 2; l < hp.n_text_layer; l++ )
			for( int h = 0; h < hp.n_text_head; h++ ) { heads.push_back( l ); heads.push_back( h ); }
	const int nHeads = (int)heads.size() / 2;
	const int layer0 = heads[ 0 ], layer1 = heads[ heads.size() - 2 ];
	std::vector<int32_t> rowOff( (size_t)batch ), R( (size_t)batch );
	for( int b = 0; b < batch; b++ )
	{
		const int32_t* const row = tokens + (size_t)b * nMax;
		const int len = lens[ b ];
		if( len < 3 || len > nMax ) { setError( "align_tokens: a window's length is outside [3, nMax]" ); return WH_E_INVALIDARG; }
		WH_CHECK( checkTokens( hp, row, len, "align_tokens" ) );
		int p = -1;
		for( int i = 0; i < len && p < 0; i++ )
			if( row[ i ] == tnot ) p = i;
		if( p < 1 || p + 3 > len ) { setError( "align_tokens: a window needs [sot sequence, no-timestamps, text..., eot] with at least one text token" ); return WH_E_INVALIDARG; }
		if( nKeys[ b ] < 1 || nKeys[ b ] > c->T ) { setError( "align_tokens: a window's key count is outside [1, audio context]" ); return WH_E_INVALIDARG; }
		rowOff[ (size_t)b ] = p;
		R[ (size_t)b ] = len - 1 - p;
	}
	hipStream_t st = c->stream;
	// buffers of the feature: first use, grown to the largest call (never part of a captured graph)
	const int nCap = layer1 - layer0 + 1;
	const int64_t rowsAll = (int64_t)batch * nMax;
	WH_CHECK( c->grow( c->alignQ, nCap * rowsAll * d, wh_context::DONT_CARE, "alignQ" ) );
	WH_CHECK( c->grow( c->alignM, rowsAll * c->T, wh_context::DONT_CARE, "alignM" ) );
	WH_CHECK( c->grow( c->alignStats, rowsAll * nHeads * 2, wh_context::DONT_CARE, "alignStats" ) );
	WH_CHECK( c->grow( c->alignFrames, rowsAll, wh_context::DONT_CARE, "alignFrames" ) );
	// the head list and the per-window sizes travel through the pinned staging's window area (free between encodes), like the tokens: nothing
	// the copy reads dies with an early return
	const int64_t metaInts = 2ll * nHeads + 4ll * batch;
	if( metaInts > wh_context::PIN_WINDOWS ) { setError( "align_tokens: too many heads and windows for one call" ); return WH_E_BOUNDS; }
	WH_CHECK( c->grow( c->alignMeta, metaInts, wh_context::DONT_CARE, "alignMeta" ) );
	c->alignBatch = 0;	   // a call that fails leaves nothing for wh_debug_read
	int* const headsDev = c->alignMeta, * const lensDev = headsDev + 2 * nHeads, * const keysDev = lensDev + batch, * const offDev = keysDev + batch, * const rDev = offDev + batch;

	int32_t* const stTok = c->pinTokens();
	WH_HIP( hipStreamSynchronize( st ) );	  // the staging may still be read by an earlier enqueue
	for( int b = 0; b < batch; b++ )
		for( int i = 0; i < nMax; i++ ) stTok[ (size_t)b * nMax + i ] = i < lens[ b ] ? tokens[ (size_t)b * nMax + i ] : 0;
	WH_HIP( hipMemcpyAsync( c->tokensDev, stTok, sizeof( int32_t ) * rowsAll, hipMemcpyHostToDevice, st ) );
	{
		int32_t* const stMeta = c->pinned;
		memcpy( stMeta, heads.data(), sizeof( int32_t ) * heads.size() );
		int32_t* const stWin = stMeta + 2 * nHeads;
		for( int b = 0; b < batch; b++ )
		{
			stWin[ b ] = lens[ b ];
			stWin[ batch + b ] = nKeys[ b ];
			stWin[ 2 * batch + b ] = rowOff[ (size_t)b ];
			stWin[ 3 * batch + b ] = R[ (size_t)b ];
		}
		WH_HIP( hipMemcpyAsync( c->alignMeta, stMeta, sizeof( int32_t ) * (size_t)metaInts, hipMemcpyHostToDevice, st ) );
	}

	// one teacher-forced pass of the multi-token decoder graph; the hook keeps the query rows of the selected layers and ends the pass behind the last one
	AlignHook hook = { layer0, layer1, c->alignQ, rowsAll * d };
	c->alignHook = &hook;
	const int rcGraph = decodeGraph( c, batch, nMax, 0, false );
	c->alignHook = nullptr;
	WH_CHECK( rcGraph );

	AlignArgs a = {};
	a.q = c->alignQ; a.k = c->crossK; a.qLayerStride = rowsAll * d; a.kLayerStride = (long long)c->maxBatch * c->T * d;
	a.qLayer0 = layer0; a.nLayers = hp.n_text_layer; a.H = hp.n_text_head; a.keyStride = c->T;
	a.heads = headsDev; a.nHeads = nHeads; a.rows = lensDev; a.keys = keysDev;
	a.windows = batch; a.nMax = nMax; a.keyMax = c->T; a.stats = c->alignStats; a.M = c->alignM;
	WH_CHECK( launchAlignMatrix( a, st ) );

	DtwArgs g = {};
	g.x = c->alignM; g.windowStride = (long long)nMax * c->T; g.rowStride = c->T; g.negate = 1; g.rowOff = offDev;
	g.R = rDev; g.keys = keysDev; g.rowMax = nMax; g.keyMax = c->T; g.frames = c->alignFrames; g.frameStride = nMax;
	WH_CHECK( launchDtw( g, batch, st ) );

	WH_HIP( hipMemcpyAsync( framesHost, c->alignFrames, sizeof( int32_t ) * rowsAll, hipMemcpyDeviceToHost, st ) );
	WH_HIP( hipStreamSynchronize( st ) );
	c->alignBatch = batch; c->alignNMax = nMax; c->alignLayer0 = layer0; c->alignLayer1 = layer1;
	return 0;
}

// Teacher-forced scores of given rows (include/whisper_hip.h; DESIGN.md section 7 "Scoring"): the pass of wh_align_tokens carried through every layer and the
// final LayerNorm, then the vocabulary product of the rows that predict a scored token only, chunk by chunk, each chunk reduced to 16 bytes per row.
int wh_score_tokens( wh_context* c, int batch, const int32_t* tokens, const int32_t* lens, const int32_t* firstScored, int nMax, wh_token_score* outHost )
{
	if( !c || !tokens || !lens || !firstScored || !outHost || batch <= 0 || nMax <= 0 ) { setError( "score_tokens: bad argument" ); return WH_E_INVALIDARG; }
	if( c->hyp != 1 ) { setError( "score_tokens: greedy contexts only (one hypothesis per window)" ); return WH_E_INVALIDARG; }
	if( c->flags & WH_FLAG_PARITY_EXACT ) { setError( "score_tokens: not under WH_FLAG_PARITY_EXACT" ); return WH_E_INVALIDARG; }
	if( !c->encoded ) { setError( "score_tokens: wh_encode has not run" ); return WH_E_NOT_READY; }
	if( batch > c->lastEncBatch ) { setError( "score_tokens: more windows than the last wh_encode filled" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	const wh_model* m = c->m;
	const wh_hparams& hp = m->hp;
	const int d = hp.n_text_state;
	if( nMax > AL_MAX_ROWS || nMax > hp.n_text_ctx || (int64_t)batch * nMax > c->pinTokenCap() ) { setError( "score_tokens: too many tokens per window" ); return WH_E_BOUNDS; }
	if( 3ll * batch > wh_context::PIN_WINDOWS ) { setError( "score_tokens: too many windows for one call" ); return WH_E_BOUNDS; }
	// per window: where its rows begin among the gathered ones
	std::vector<int32_t> off( (size_t)batch );
	int64_t rowsScored = 0;
	for( int b = 0; b < batch; b++ )
	{
		const int len = lens[ b ], first = firstScored[ b ];
		if( len < 2 || len > nMax ) { setError( "score_tokens: a window's length is outside [2, nMax]" ); return WH_E_INVALIDARG; }
		if( first < 1 || first >= len ) { setError( "score_tokens: a window's first scored entry is outside [1, its length)" ); return WH_E_INVALIDARG; }
		WH_CHECK( checkTokens( hp, tokens + (size_t)b * nMax, len, "score_tokens" ) );
		off[ (size_t)b ] = (int32_t)rowsScored;
		rowsScored += len - first;
	}
	hipStream_t st = c->stream;
	// buffers of the feature: first use, grown to the largest call (never part of a captured graph). The logits hold one chunk of rows.
	const int64_t rowsAll = (int64_t)batch * nMax;
	// (the logits are sized for a whole chunk at once: grown call by call, the doubling of grow() would pass the cap the option sets)
	const int chunk = std::max( 1, std::min( g_opt.scoreChunkRows, 4096 ) );
	WH_CHECK( c->grow( c->scoreRows, rowsScored * d, wh_context::DONT_CARE, "scoreRows" ) );
	WH_CHECK( c->grow( c->scoreLogits, (int64_t)chunk * hp.n_vocab, wh_context::DONT_CARE, "scoreLogits" ) );
	WH_CHECK( c->grow( c->scoreOut, rowsScored, wh_context::DONT_CARE, "scoreOut" ) );
	WH_CHECK( c->grow( c->scoreTargets, rowsScored, wh_context::DONT_CARE, "scoreTargets" ) );
	WH_CHECK( c->grow( c->scoreMeta, 3ll * batch, wh_context::DONT_CARE, "scoreMeta" ) );

	// the tokens and the per-window sizes travel through the pinned staging like wh_align_tokens': nothing the copies read dies with an early return
	int32_t* const stTok = c->pinTokens();
	WH_HIP( hipStreamSynchronize( st ) );	  // the staging may still be read by an earlier enqueue
	for( int b = 0; b < batch; b++ )
		for( int i = 0; i < nMax; i++ ) stTok[ (size_t)b * nMax + i ] = i < lens[ b ] ? tokens[ (size_t)b * nMax + i ] : 0;
	WH_HIP( hipMemcpyAsync( c->tokensDev, stTok, sizeof( int32_t ) * rowsAll, hipMemcpyHostToDevice, st ) );
	{
		int32_t* const stMeta = c->pinned;
		for( int b = 0; b < batch; b++ )
		{
			stMeta[ b ] = firstScored[ b ];
			stMeta[ batch + b ] = lens[ b ];
			stMeta[ 2 * batch + b ] = off[ (size_t)b ];
		}
		WH_HIP( hipMemcpyAsync( c->scoreMeta, stMeta, sizeof( int32_t ) * 3 * (size_t)batch, hipMemcpyHostToDevice, st ) );
	}

	// one teacher-forced pass of the multi-token decoder graph; the hook ends it behind the final LayerNorm of all rows
	c->scoreHook = true;
	const int rcGraph = decodeGraph( c, batch, nMax, 0, false );
	c->scoreHook = false;
	WH_CHECK( rcGraph );

	WH_CHECK( profiled( c, KC_SAMPLE, 0.0, 4.0 * rowsScored * d,
		[ & ]() { return launchGatherScoreRows( c->dxn, c->tokensDev, c->scoreMeta, batch, nMax, d, c->scoreRows, c->scoreTargets, st ); } ) );
	// The vocabulary product in chunks of rows, each followed by its reduction. Always the M-tiled kernel (the choice decodeGraph makes beyond 128 sequences): its
	// sums do not depend on how many rows a launch has, so the records are the same bits whatever the chunk size -- the decode products pick a kernel by row count.
	for( int64_t r0 = 0; r0 < rowsScored; r0 += chunk )
	{
		const int rows = (int)std::min<int64_t>( chunk, rowsScored - r0 );
		GemmArgs g = plainGemm( c->scoreRows + r0 * d, m->at<f16>( m->L.te ), rows, hp.n_vocab, d );
		g.epi = EPI_F32; g.out32 = c->scoreLogits; g.ldc = hp.n_vocab;
		WH_CHECK( gemmP( c, g, false, false ) );	  // (accounted under the tiled products' class, which nothing else of a decoder pass uses: wh_profile_read splits the call)
		WH_CHECK( profiled( c, KC_SAMPLE, 20.0 * rows * hp.n_vocab, 4.0 * rows * hp.n_vocab,
			[ & ]() { return launchTokenScores( c->scoreLogits, hp.n_vocab, rows, hp.n_vocab, c->scoreTargets + r0, c->scoreOut + r0, st ); } ) );
	}

	std::vector<TokenScore> got( (size_t)rowsScored );
	WH_HIP( hipMemcpyAsync( got.data(), c->scoreOut, sizeof( TokenScore ) * (size_t)rowsScored, hipMemcpyDeviceToHost, st ) );
	WH_HIP( hipStreamSynchronize( st ) );
	memset( outHost, 0, sizeof( wh_token_score ) * (size_t)rowsAll );
	for( int b = 0; b < batch; b++ )
		for( int i = firstScored[ b ]; i < lens[ b ]; i++ )
		{
			const TokenScore& s = got[ (size_t)off[ (size_t)b ] + (size_t)( i - firstScored[ b ] ) ];
			outHost[ (size_t)b * nMax + i ] = wh_token_score{ s.logprob, s.bestLogprob, s.best, s.rank };
		}
	return 0;
}

}	// extern "C"
