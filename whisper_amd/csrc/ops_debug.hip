// Diagnostics and development aids: the profiler's switches, wh_debug_read, the op-level entry points (wh_op_*) and the micro-benchmarks of
// wh_debug_probe with their kernels.
#include "runtime.h"
#include "gemm_launch.h"

namespace
{
	__global__ void probeEmpty( int* p ) { if( p && threadIdx.x == 0xFFFF ) *p = 1; }

	// Device memory of the op-level entry points, which have no context to own it: one buffer per (device, key), allocated and filled on first use,
	// reused by every later call with that key and kept for the life of the process.
	struct OpScratch
	{
		struct Key
		{
			int device;
			const void* key;
			bool operator<( const Key& o ) const { return device != o.device ? device < o.device : key < o.key; }
		};
		std::mutex mx;
		std::map<Key, void*> bufs;
		template<class F> int get( const void* key, size_t bytes, void** out, F&& fill )
		{
			int dev = 0;
			WH_HIP( hipGetDevice( &dev ) );
			std::lock_guard<std::mutex> lk( mx );
			void*& p = bufs.emplace( Key{ dev, key }, nullptr ).first->second;
			if( !p )
			{
				void* v = nullptr;
				WH_HIP( hipMalloc( &v, bytes ) );
				const int rc = fill( v );
				if( rc != 0 ) { (void)hipFree( v ); return rc; }
				p = v;
			}
			*out = p;
			return 0;
		}
	};
	OpScratch g_opSplitK, g_opExpTable;

	// what a probe run holds: released when wh_debug_probe returns, on its error paths too
	struct ProbeEvent
	{
		hipEvent_t ev = nullptr;
		int create() { WH_HIP( hipEventCreate( &ev ) ); return 0; }
		~ProbeEvent() { if( ev ) (void)hipEventDestroy( ev ); }
		operator hipEvent_t() const { return ev; }
	};
	struct ProbeMemory
	{
		std::vector<void*> owned;
		template<class T> int alloc( T** p, size_t bytes )
		{
			WH_HIP( hipMalloc( (void**)p, bytes ) );
			owned.push_back( *p );
			return 0;
		}
		~ProbeMemory()
		{
			for( void* p : owned ) (void)hipFree( p );
		}
	};
}

extern "C" {

int wh_profile_enable( wh_context* c, int on )
{
	if( !c ) return WH_E_INVALIDARG;
	WH_BIND( c->m );
	c->prof.reset();
	c->prof.on = on != 0;
	if( c->prof.on )
	{
		// calibration: what an event pair around a launch measures when the kernel does nothing (the first launch of a
		// kernel loads its code object: keep that out of the average)
		for( int i = 0; i < 4; i++ ) hipLaunchKernelGGL( probeEmpty, dim3( 1 ), dim3( 64 ), 0, c->stream, (int*)nullptr );
		WH_HIP( hipStreamSynchronize( c->stream ) );
		for( int i = 0; i < 64; i++ )
			WH_CHECK( profiled( c, KC_EVENT_PAIR, 0.0, 0.0, [ & ]() { hipLaunchKernelGGL( probeEmpty, dim3( 1 ), dim3( 64 ), 0, c->stream, (int*)nullptr ); return 0; } ) );
	}
	return 0;
}

int wh_profile_read( wh_context* c, wh_profile_entry* out, int cap, int* count )
{
	if( !c || !count ) return WH_E_INVALIDARG;
	WH_BIND( c->m );
	WH_HIP( hipStreamSynchronize( c->stream ) );
	c->prof.resolve();
	int n = 0;
	for( int i = 0; i < KC_COUNT; i++ )
	{
		if( c->prof.calls[ i ] == 0 ) continue;
		if( out && n < cap )
		{
			wh_profile_entry& e = out[ n ];
			memset( &e, 0, sizeof( e ) );
			snprintf( e.name, sizeof( e.name ), "%s", kernelClassNames[ i ] );
			e.calls = c->prof.calls[ i ];
			e.ms = c->prof.ms[ i ];
			e.flops = c->prof.flops[ i ];
			e.bytes = c->prof.bytes[ i ];
		}
		n++;
	}
	*count = n;
	return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// debug reads
// ------------------------------------------------------------------------------------------------------------------
static int readHeadMajor( wh_context* c, const f16* src, int batch, int rows, int rowStride, float* dst )
{
	// [b][h][rowStride][64] FP16 -> [b][rows][H*64] FP32
	const int H = c->m->hp.n_audio_head, d = H * HEAD_DIM;
	std::vector<uint16_t> tmp( (size_t)batch * H * rowStride * HEAD_DIM );
	WH_HIP( hipStreamSynchronize( c->stream ) );
	WH_HIP( hipMemcpy( tmp.data(), src, tmp.size() * 2, hipMemcpyDeviceToHost ) );
	for( int b = 0; b < batch; b++ )
		for( int h = 0; h < H; h++ )
			for( int t = 0; t < rows; t++ )
				for( int j = 0; j < HEAD_DIM; j++ )
					dst[ ( (size_t)b * rows + t ) * d + h * HEAD_DIM + j ] = f16BitsToF32( tmp[ ( ( (size_t)b * H + h ) * rowStride + t ) * HEAD_DIM + j ] );
	return 0;
}

int wh_debug_read( wh_context* c, const char* what, int layer, int rows, float* dstHost, int64_t dstCapFloats )
{
	if( !c || !what || !dstHost ) return WH_E_INVALIDARG;
	WH_BIND( c->m );
	const wh_hparams& hp = c->m->hp;
	const int d = hp.n_audio_state;
	const int batch = c->lastEncBatch;
	const int seqs = c->lastBatch;
	const std::string w = what;
	if( w == "exp-table" )
	{
		// the arena's copy of the reference's exponential table (non-positive arguments), as FP32 values
		if( dstCapFloats < EXP_TABLE_ENTRIES ) return WH_E_BOUNDS;
		std::vector<uint16_t> tmp( EXP_TABLE_ENTRIES );
		WH_HIP( hipMemcpy( tmp.data(), c->m->at<f16>( c->m->L.expTab ), EXP_TABLE_ENTRIES * 2, hipMemcpyDeviceToHost ) );
		for( int i = 0; i < EXP_TABLE_ENTRIES; i++ ) dstHost[ i ] = f16BitsToF32( tmp[ (size_t)i ] );
		return 0;
	}
	if( w == "exact-gelu-table" || w == "exact-exp-table" )
	{
		// WH_FLAG_PARITY_EXACT's copies of ggml_init's tables, all 65536 entries, as FP32 values
		if( dstCapFloats < 65536 ) return WH_E_BOUNDS;
		WH_CHECK( exactTables( c ) );
		std::vector<uint16_t> tmp( 65536 );
		WH_HIP( hipMemcpy( tmp.data(), w == "exact-gelu-table" ? c->ex.gelu : c->ex.expt, 65536 * 2, hipMemcpyDeviceToHost ) );
		for( int i = 0; i < 65536; i++ ) dstHost[ i ] = f16BitsToF32( tmp[ (size_t)i ] );
		return 0;
	}
	if( w.compare( 0, 6, "exact:" ) == 0 )
	{
		// a buffer of the exact-order encoder as the last wh_encode left it (first chunk of windows): x, cur, q, k, v, kqv [windows][n_ctx][d], h [..][4 d], conv1 [..][2 n_ctx][d]
		const std::string n = w.substr( 6 );
		const wh_context::Exact& e = c->ex;
		const float* src = n == "x" ? e.x : n == "cur" ? e.cur : n == "q" ? e.q : n == "k" ? e.k : n == "v" ? e.v : n == "kqv" ? e.kqv : n == "h" ? e.h : n == "conv1" ? e.conv1 : nullptr;
		if( !src ) { setError( "debug_read: no such exact-mode buffer (or the mode has not run)" ); return WH_E_NOT_READY; }
		const int64_t count = (int64_t)std::min( batch, e.encWindows ) * c->T * d * ( n == "h" ? 4 : n == "conv1" ? 2 : 1 );
		if( dstCapFloats < count ) return WH_E_BOUNDS;
		WH_HIP( hipStreamSynchronize( c->stream ) );
		WH_HIP( hipMemcpy( dstHost, src, (size_t)count * 4, hipMemcpyDeviceToHost ) );
		return 0;
	}
	if( w == "logits" || w == "probs" )
	{
		// what the LAST decode step left: logits (or, after wh_decode with probsHost / the sampler, probabilities) of every sequence, [seqs][n_vocab]
		const int64_t n = (int64_t)seqs * hp.n_vocab;
		if( n <= 0 || dstCapFloats < n ) return WH_E_BOUNDS;
		WH_HIP( hipStreamSynchronize( c->stream ) );
		WH_HIP( hipMemcpy( dstHost, w == "logits" ? c->logits : c->probs, (size_t)n * 4, hipMemcpyDeviceToHost ) );
		return 0;
	}
	if( w == "cross-k1" || w == "cross-v1" )
	{
		// ONE window (index `rows`) of a layer's cross-attention cache: [n_ctx][d] -- contexts of hundreds of windows
		if( layer < 0 || layer >= hp.n_text_layer || rows < 0 || rows >= batch || dstCapFloats < (int64_t)c->T * d ) return WH_E_BOUNDS;
		const f16* base = ( w == "cross-k1" ? c->crossK : c->crossV ) + ( (int64_t)layer * c->maxBatch + rows ) * c->T * d;
		return readHeadMajor( c, base, 1, c->T, c->T, dstHost );
	}
	if( w == "encode-out" )
	{
		// the FP16 LayerNorm output that feeds the cross-attention projection (of a batch the encoder took in one chunk)
		if( batch > c->encChunk ) { setError( "debug_read: encode-out holds the last encoder chunk only" ); return WH_E_BOUNDS; }
		const int64_t n = (int64_t)batch * c->T * d;
		if( dstCapFloats < n ) return WH_E_BOUNDS;
		std::vector<uint16_t> tmp( (size_t)n );
		WH_HIP( hipStreamSynchronize( c->stream ) );
		WH_HIP( hipMemcpy( tmp.data(), c->xn, (size_t)n * 2, hipMemcpyDeviceToHost ) );
		for( int64_t i = 0; i < n; i++ ) dstHost[ i ] = f16BitsToF32( tmp[ (size_t)i ] );
		return 0;
	}
	auto readF16 = [ & ]( const f16* src, int64_t n ) -> int
	{
		if( !src ) { setError( "debug_read: nothing captured (set WH_FLAG_DEBUG_CAPTURE before the call that produces it)" ); return WH_E_NOT_READY; }
		if( dstCapFloats < n ) return WH_E_BOUNDS;
		std::vector<uint16_t> tmp( (size_t)n );
		WH_HIP( hipStreamSynchronize( c->stream ) );
		WH_HIP( hipMemcpy( tmp.data(), src, (size_t)n * 2, hipMemcpyDeviceToHost ) );
		for( int64_t i = 0; i < n; i++ ) dstHost[ i ] = f16BitsToF32( tmp[ (size_t)i ] );
		return 0;
	};
	if( w == "enc.temp1" )
	{
		// conv1 + bias + GELU, time-major [batch][2*n_ctx][d] (the reference's tensor is [d][2*n_ctx]); padding rows dropped
		if( !c->capTemp1 ) return readF16( nullptr, 0 );
		const int64_t rowsT = 2ll * c->T;
		if( dstCapFloats < batch * rowsT * d ) return WH_E_BOUNDS;
		std::vector<uint16_t> tmp( (size_t)( batch * c->conv1Stride ) );
		WH_HIP( hipStreamSynchronize( c->stream ) );
		WH_HIP( hipMemcpy( tmp.data(), c->capTemp1, tmp.size() * 2, hipMemcpyDeviceToHost ) );
		for( int b = 0; b < batch; b++ )
			for( int64_t i = 0; i < rowsT * d; i++ ) dstHost[ b * rowsT * d + i ] = f16BitsToF32( tmp[ (size_t)( b * c->conv1Stride + d + i ) ] );
		return 0;
	}
	if( w == "enc.layer0.in" )
	{
		const int64_t n = (int64_t)batch * c->T * d;
		if( !c->capLayer0In ) return readF16( nullptr, 0 );
		if( dstCapFloats < n ) return WH_E_BOUNDS;
		WH_HIP( hipStreamSynchronize( c->stream ) );
		WH_HIP( hipMemcpy( dstHost, c->capLayer0In, (size_t)n * 4, hipMemcpyDeviceToHost ) );
		return 0;
	}
	if( w == "enc-KQV" ) return readF16( c->capEncKqv, (int64_t)batch * c->T * d );	   // layer 0, [batch][n_ctx][d] (heads side by side)
	if( w == "dec-KQV" ) return readF16( c->capDecKqvSelf, (int64_t)c->capDecRows * d );   // layer 0 self-attention output, rows of the last wh_decode
	if( w == "dec-KQV#2" ) return readF16( c->capDecKqvCross, (int64_t)c->capDecRows * d );
	if( const int rcAlign = alignDebugRead( c, w, layer, dstHost, dstCapFloats ); rcAlign != 1 ) return rcAlign;
	if( layer < 0 || layer >= hp.n_text_layer ) return WH_E_BOUNDS;
	if( w == "cross-k" || w == "cross-v" )
	{
		if( dstCapFloats < (int64_t)batch * c->T * d ) return WH_E_BOUNDS;
		const f16* base = ( w == "cross-k" ? c->crossK : c->crossV ) + (int64_t)layer * c->maxBatch * c->T * d;
		return readHeadMajor( c, base, batch, c->T, c->T, dstHost );
	}
	if( w == "self-k" || w == "self-v" )
	{
		if( rows <= 0 || rows > hp.n_text_ctx || dstCapFloats < (int64_t)seqs * rows * d ) return WH_E_BOUNDS;
		const f16* base = ( w == "self-k" ? c->selfK : c->selfV ) + (int64_t)layer * c->maxSeq * hp.n_text_ctx * d;
		return readHeadMajor( c, base, seqs, rows, hp.n_text_ctx, dstHost );
	}
	setError( "debug_read: unknown item" );
	return WH_E_INVALIDARG;
}

// ==================================================================================================================
// op-level entry points
// ==================================================================================================================
int wh_op_mul_mat( void* stream, const void* aF16, const void* wF16, const float* bias, const float* residual, float* out, int M, int N, int K )
{
	GemmArgs g = plainGemm( (const f16*)aF16, (const f16*)wF16, M, N, K );
	g.epi = EPI_F32; g.bias = bias; g.res = residual; g.out32 = out;
	if( M > 32 && M <= GEMV_FUSED_MAX_ROWS && N <= 2048 && K >= 2048 )
	{
		// option dec_split needs room for its eight partial tiles: no context here, so the op-level entry keeps one buffer per (device, stream) -- calls on
		// different streams never share partial tiles, calls on one stream are ordered (the decoder passes its context's buffer)
		void* tiles = nullptr;
		WH_CHECK( g_opSplitK.get( stream, 8ull * GEMV_FUSED_MAX_ROWS * 2048 * sizeof( float ), &tiles, []( void* ) { return 0; } ) );
		g.splitScratch = (float*)tiles;
	}
	// the same choice the decoder makes: up to 32 rows go to the gemv when K allows it
	if( M <= GEMV_MAX_ROWS && ( K % 128 ) == 0 ) return launchGemv( g, (hipStream_t)stream );	   // the op-level entry is the decode-step product: up to 512 rows on the weight-streaming kernels
	return M <= 32 ? launchGemmSkinny( g, (hipStream_t)stream ) : launchGemm( g, (hipStream_t)stream );
}

int wh_op_mul_mat_gelu( void* stream, const void* aF16, const void* wF16, const float* bias, void* outF16, int M, int N, int K )
{
	if( !bias ) { setError( "mul_mat_gelu: bias is required" ); return WH_E_INVALIDARG; }
	GemmArgs g = plainGemm( (const f16*)aF16, (const f16*)wF16, M, N, K );
	g.epi = EPI_F16_GELU; g.bias = bias; g.out16 = (f16*)outF16;
	if( M <= GEMV_MAX_ROWS && ( K % 128 ) == 0 ) return launchGemv( g, (hipStream_t)stream );	   // the op-level entry is the decode-step product: up to 512 rows on the weight-streaming kernels
	return M <= 32 ? launchGemmSkinny( g, (hipStream_t)stream ) : launchGemm( g, (hipStream_t)stream );
}

// ---- the encoder's fused products as wh_encode builds them (encode.hip), through the same chooser. Thin, but everything the launchers cannot see and a kernel
// would turn into an address is checked here: a call either describes buffers the product stays inside, or launches nothing.
int wh_op_gemm_encoder( void* stream, const wh_gemm_encoder_args* p, int32_t* family, int32_t* wideEpi )
{
	const auto bad = []( const char* what ) { setError( std::string( "gemm_encoder: " ) + what ); return (int)WH_E_INVALIDARG; };
	if( !p || !p->a || !p->w ) return bad( "null argument" );
	if( p->M <= 0 || p->N <= 0 || p->K <= 0 || p->lda <= 0 || p->Mb <= 0 || p->aBatchStride < 0 || p->cBatchStride < 0 ) return bad( "M, N, K, lda and Mb must be positive, the strides non-negative" );
	const bool segmented = p->Mb < p->M;
	if( segmented && ( p->M % p->Mb ) != 0 ) return bad( "M must be whole segments of Mb rows" );
	GemmArgs g = plainGemm( (const f16*)p->a, (const f16*)p->w, p->M, p->N, p->K );
	g.lda = p->lda; g.Mb = p->Mb; g.aBatchStride = p->aBatchStride;
	g.ldc = p->ldc; g.cBatchStride = p->cBatchStride;
	g.epi = p->epi; g.bias = p->bias; g.scale = p->scale;
	const long long d = 64ll * p->H;
	switch( p->epi )
	{
	case EPI_F32:
	case EPI_F16_GELU:
		if( p->epi == EPI_F32 ? !p->out32 : ( !p->out16 || !p->bias ) ) return bad( "the epilogue's output (and the GELU's bias) must not be null" );
		if( p->ldc < p->N || ( segmented && p->cBatchStride < (long long)p->Mb * p->ldc ) ) return bad( "ldc >= N and output segments that do not overlap" );
		g.res = p->epi == EPI_F32 ? p->res : nullptr; g.out32 = p->out32; g.out16 = (f16*)p->out16;
		break;
	case EPI_CONV2:
		if( !p->out32 || !p->bias || !p->pe ) return bad( "conv2 needs out32, bias and pe" );
		if( p->ldc < p->N ) return bad( "ldc >= N" );
		g.pe = p->pe; g.out32 = p->out32;
		break;
	case EPI_QKV_ENC:
		if( !p->q || !p->k || !p->v || !p->bias ) return bad( "Q/K/V needs q, k, v and bias" );
		if( p->H <= 0 || p->N != 3 * d ) return bad( "Q/K/V: N must be 3 * 64 * H" );
		if( p->T <= 0 || ( p->M % p->T ) != 0 ) return bad( "M % T must be 0" );
		if( p->Tpad < p->T || ( p->Tpad % 16 ) != 0 ) return bad( "Tpad must be a multiple of 16 and at least T" );
		g.q = (f16*)p->q; g.k = (f16*)p->k; g.v = (f16*)p->v;
		g.T = p->T; g.Tpad = p->Tpad; g.H = p->H; g.B = p->M / p->T;
		break;
	case EPI_CROSS_KV:
		if( !p->k || !p->v || !p->bias ) return bad( "cross-K/V needs k, v and bias" );
		if( p->H <= 0 || ( p->N % ( 2 * d ) ) != 0 ) return bad( "cross-K/V: N % ( 2 * 64 * H ) must be 0" );
		if( p->T <= 0 || ( p->M % p->T ) != 0 ) return bad( "M % T must be 0" );
		if( p->B < p->M / p->T ) return bad( "cross-K/V: B must hold the M / T windows" );
		g.k = (f16*)p->k; g.v = (f16*)p->v;
		g.T = p->T; g.H = p->H; g.B = p->B;
		break;
	default:
		return bad( "unknown epilogue" );
	}
	WH_CHECK( checkGemmArgs( g ) );
	const int fam = chooseGemmFamily( g );
	WH_CHECK( launchGemm( g, (hipStream_t)stream ) );
	if( family ) *family = fam;
	if( wideEpi ) *wideEpi = t_gemmWideEpi;
	return 0;
}

int wh_op_mel_to_conv_input( void* stream, const float* melDev, int64_t melStride, int64_t melLen, const int32_t* offsetsHost, const wh_mel_window* windowsHost,
	void* x16, int64_t xBatchStride, int nMels, int rows, int batch )
{
	const auto bad = []( const char* what ) { setError( std::string( "mel_to_conv_input: " ) + what ); return (int)WH_E_INVALIDARG; };
	if( !x16 || nMels <= 0 || rows <= 0 || batch <= 0 || batch > 4096 ) return bad( "bad argument" );
	if( xBatchStride < ( (int64_t)rows + 2 ) * nMels ) return bad( "xBatchStride must hold rows + 2 rows" );
	static_assert( sizeof( MelWindow ) == 24 && sizeof( wh_mel_window ) == 24, "window descriptor layout" );
	std::vector<MelWindow> wins;
	std::vector<int32_t> offs;
	if( windowsHost )
	{
		for( int i = 0; i < batch; i++ )
		{
			if( windowsHost[ i ].melDev && ( windowsHost[ i ].melLen <= 0 || windowsHost[ i ].offset < 0 ) ) return bad( "bad window" );
			wins.push_back( MelWindow{ windowsHost[ i ].melDev, (long long)windowsHost[ i ].melLen, windowsHost[ i ].offset, 0 } );
		}
	}
	else
	{
		if( !melDev || melLen <= 0 || melStride < 0 ) return bad( "bad spectrogram" );
		for( int i = 0; i < batch; i++ )
		{
			if( offsetsHost && offsetsHost[ i ] < 0 ) return bad( "negative offset" );
			offs.push_back( offsetsHost ? offsetsHost[ i ] : 0 );
		}
	}
	ProbeMemory mem;
	MelWindow* winsDev = nullptr;
	int32_t* offsDev = nullptr;
	if( windowsHost )
	{
		WH_CHECK( mem.alloc( &winsDev, sizeof( MelWindow ) * batch ) );
		WH_HIP( hipMemcpy( winsDev, wins.data(), sizeof( MelWindow ) * batch, hipMemcpyHostToDevice ) );
	}
	else
	{
		WH_CHECK( mem.alloc( &offsDev, sizeof( int32_t ) * batch ) );
		WH_HIP( hipMemcpy( offsDev, offs.data(), sizeof( int32_t ) * batch, hipMemcpyHostToDevice ) );
	}
	WH_CHECK( launchMelToConvInput( melDev, melStride, melLen, offsDev, winsDev, (f16*)x16, xBatchStride, nMels, rows, batch, (hipStream_t)stream ) );
	WH_HIP( hipStreamSynchronize( (hipStream_t)stream ) );	   // the descriptors are released on return
	return 0;
}

int wh_op_layer_norm( void* stream, const float* x, const float* w, const float* b, void* outF16, int rows, int d )
{
	return launchLayerNorm( x, w, b, (f16*)outF16, rows, d, (hipStream_t)stream );
}

int wh_op_flash_attention( void* stream, const void* q, const void* k, const void* vT, void* out, int batch, int heads, int nCtx )
{
	// no model here: the op-level entry keeps its own copy of the exponential's table per device (built like wh_model_finalize builds the arena's)
	const f16* expTab = nullptr;
	if( g_tuning & TUNE_ATTN_ENC_TABLE )
	{
		void* tab = nullptr;
		WH_CHECK( g_opExpTable.get( nullptr, EXP_TABLE_ENTRIES * 2, &tab, []( void* dst ) -> int
		{
			std::vector<_Float16> tab( EXP_TABLE_ENTRIES );
			for( uint32_t i = 0; i < (uint32_t)EXP_TABLE_ENTRIES; i++ )
			{
				const uint16_t bits = (uint16_t)( i | 0x8000u );
				_Float16 h;
				memcpy( &h, &bits, 2 );
				tab[ i ] = (_Float16)expf( (float)h );
			}
			WH_HIP( hipMemcpy( dst, tab.data(), EXP_TABLE_ENTRIES * 2, hipMemcpyHostToDevice ) );
			return 0;
		} ) );
		expTab = (const f16*)tab;
	}
	return launchAttentionEnc( (const f16*)q, (const f16*)k, (const f16*)vT, (f16*)out, batch, heads, nCtx, roundUp( nCtx, 256 ), false, expTab, (hipStream_t)stream );
}

int wh_op_decoder_attention( void* stream, const void* qF16, const void* kCache, const void* vCache, void* outF16, int sequences, int heads,
	int nTok, int nKeys, int keyStride, int causal, int nPast, int group, int parityThreads )
{
	DecAttnArgs a = {};
	a.q = (const f16*)qF16; a.kc = (const f16*)kCache; a.vc = (const f16*)vCache; a.out = (f16*)outF16;
	a.batch = sequences; a.H = heads; a.nTok = nTok; a.nKeys = nKeys; a.keyStride = keyStride;
	a.causal = causal; a.nPast = nPast; a.group = group; a.parityThreads = parityThreads;
	return launchAttentionDec( a, (hipStream_t)stream );
}

int wh_op_decoder_cross_attention( void* stream, const float* x, const float* lnW, const float* lnB, const void* qW, const float* qB, float qScale,
	const void* kCache, const void* vCache, void* outF16, int sequences, int heads, int nKeys, int keyStride, int group )
{
	if( !x || !lnW || !lnB || !qW || !qB ) { setError( "decoder_cross_attention: null argument" ); return WH_E_INVALIDARG; }
	DecAttnArgs a = {};
	a.kc = (const f16*)kCache; a.vc = (const f16*)vCache; a.out = (f16*)outF16;
	a.batch = sequences; a.H = heads; a.nTok = 1; a.nKeys = nKeys; a.keyStride = keyStride;
	a.group = group;
	a.lnX = x; a.lnW = lnW; a.lnB = lnB; a.qW = (const f16*)qW; a.qB = qB; a.qScale = qScale;
	return launchAttentionDec( a, (hipStream_t)stream );
}

int wh_op_soft_max( void* stream, float* x, int rows, int cols )
{
	return launchSoftMaxRows( x, rows, cols, (hipStream_t)stream );
}

// ---- the kernels of a single-token step: the products and the split cross-attention of one stream (decode1.hip), the fused self-attention half of a
// lock-step batch (attn_dec.hip). Thin: the launchers check the shapes; what they cannot see (null pointers, a position outside the cache) is checked here.
int wh_op_gemv_small( void* stream, int M, int N, int K, int epi, int pro, const void* wF16, const void* aF16, const float* lnX, const float* lnW, const float* lnB,
	const float* part, const float* bias, const float* residual, float* out32, void* out16, void* qF16, void* kCache, void* vCache, int heads, int textCtx,
	int nPast, const int32_t* nPastDev, float scale )
{
	if( !wF16 || ( pro != 0 && pro != 1 && pro != 3 ) || ( pro == 0 && !aF16 ) || ( pro == 1 && ( !lnX || !lnW || !lnB ) ) || ( pro == 3 && !part ) )
	{
		setError( "gemv_small: null operand, or a prologue other than 0 (FP16 rows), 1 (LayerNorm) or 3 (cross-attention partials)" );
		return WH_E_INVALIDARG;
	}
	SmallGemvArgs a = {};
	a.g = plainGemm( (const f16*)aF16, (const f16*)wF16, M, N, K );
	a.pro = pro; a.part = part;
	a.g.lnX = lnX; a.g.lnW = lnW; a.g.lnB = lnB;
	a.g.bias = bias;
	if( epi == 0 )
	{
		if( !out32 ) { setError( "gemv_small: the FP32 epilogue needs out32" ); return WH_E_INVALIDARG; }
		a.g.epi = EPI_F32; a.g.res = residual; a.g.out32 = out32;
	}
	else if( epi == 1 )
	{
		if( !out16 || !bias ) { setError( "gemv_small: the GELU epilogue needs out16 and a bias" ); return WH_E_INVALIDARG; }
		a.g.epi = EPI_F16_GELU; a.g.out16 = (f16*)out16;
	}
	else if( epi == 2 )
	{
		// every position written must lie inside the cache: a scalar is checked here, a device array is the caller's to keep in [0, textCtx)
		if( !qF16 || !kCache || !vCache || !bias || heads < 1 || N != 3 * heads * HEAD_DIM || K != heads * HEAD_DIM || textCtx < 1 ||
			( !nPastDev && ( nPast < 0 || nPast >= textCtx ) ) )
		{
			setError( "gemv_small: the QKV epilogue needs q, both caches and a bias, N = 3 K = 3 * 64 * heads and 0 <= nPast < textCtx" );
			return WH_E_INVALIDARG;
		}
		a.g.epi = EPI_QKV_DEC; a.g.scale = scale;
		a.g.q = (f16*)qF16; a.g.k = (f16*)kCache; a.g.v = (f16*)vCache;
		a.g.H = heads; a.g.nTok = 1; a.g.nPast = nPast; a.g.nPastDev = nPastDev; a.g.textCtx = textCtx;
	}
	else
	{
		setError( "gemv_small: epilogue 0 (FP32, bias, residual), 1 (FP16 GELU) or 2 (decoder Q/K/V)" );
		return WH_E_INVALIDARG;
	}
	return launchGemvSmall( a, (hipStream_t)stream );
}

int wh_op_cross_split( void* stream, const float* x, const float* lnW, const float* lnB, const void* qW, const float* qB, float qScale, const void* kCache,
	const void* vCache, float* scores, float* splitMax, float* part, int sequences, int heads, int nKeys, int keyStride )
{
	if( !x || !lnW || !lnB || !qW || !qB || !kCache || !vCache || !scores || !splitMax || !part || heads < 1 )
	{
		setError( "cross_split: null argument" );
		return WH_E_INVALIDARG;
	}
	CrossSplitArgs a = {};
	a.lnX = x; a.lnW = lnW; a.lnB = lnB; a.qW = (const f16*)qW; a.qB = qB; a.qScale = qScale;
	a.kc = (const f16*)kCache; a.vc = (const f16*)vCache;
	a.scores = scores; a.splitMax = splitMax; a.part = part;
	a.batch = sequences; a.H = heads; a.nKeys = nKeys; a.keyStride = keyStride;
	WH_CHECK( launchCrossScores( a, (hipStream_t)stream ) );
	return launchCrossSoftmaxPV( a, (hipStream_t)stream );
}

int wh_op_self_block_dec( void* stream, const float* x, const float* lnW, const float* lnB, const void* wqkv, const float* bqkv, float scale, void* kCache,
	void* vCache, void* outF16, int sequences, int heads, int keyStride, int nPast, const int32_t* nPastDev )
{
	// a scalar position is checked here; positions in device memory are the caller's to keep in [0, keyStride)
	if( !x || !lnW || !lnB || !wqkv || !bqkv || !kCache || !vCache || !outF16 || heads < 1 || ( !nPastDev && ( nPast < 0 || nPast >= keyStride ) ) )
	{
		setError( "self_block_dec: null argument, or nPast outside [0, keyStride)" );
		return WH_E_INVALIDARG;
	}
	DecSelfArgs a = {};
	a.x = x; a.lnW = lnW; a.lnB = lnB; a.wqkv = (const f16*)wqkv; a.bqkv = bqkv; a.scale = scale;
	a.kc = (f16*)kCache; a.vc = (f16*)vCache; a.out = (f16*)outF16;
	a.batch = sequences; a.H = heads; a.keyStride = keyStride; a.nPast = nPast; a.nPastDev = nPastDev;
	return launchSelfBlockDec( a, (hipStream_t)stream );
}

int wh_op_vocab_soft_max( void* stream, const float* logits, float* probs, int rows, int cols )
{
	if( !logits || !probs || rows < 1 || cols < 1 ) { setError( "vocab_soft_max: null pointer or empty shape" ); return WH_E_INVALIDARG; }
	return launchVocabSoftMax( logits, probs, rows, cols, (hipStream_t)stream );
}

int wh_op_suppress_logits( void* stream, float* logits, int rows, int nVocab, const int32_t* ids, int count )
{
	if( !logits || rows < 1 || nVocab < 1 || count < 0 || ( count > 0 && !ids ) ) { setError( "suppress_logits: null pointer, empty shape or negative count" ); return WH_E_INVALIDARG; }
	if( count == 0 ) return 0;
	return launchSuppressLogits( logits, rows, nVocab, ids, nullptr, count, count, (hipStream_t)stream );
}

int wh_op_timestamp_rules( void* stream, float* logits, int rows, int nVocab, int tokenEot, int tokenBeg, const int32_t* fedTokensDev, int reset, int32_t* recordsDev )
{
	static_assert( sizeof( TimestampRecord ) == 4 * sizeof( int32_t ), "wh_op_timestamp_rules documents the record as four int32" );
	if( !logits || !recordsDev || ( !reset && !fedTokensDev ) || rows < 1 || nVocab < 2 || tokenBeg < 1 || tokenBeg >= nVocab || tokenEot < 0 || tokenEot >= tokenBeg ||
		reset < 0 || reset > 2 )
	{
		setError( "timestamp_rules: null pointer, empty shape, ids that are not 0 <= eot < beg < nVocab, or a reset outside 0 .. 2" );
		return WH_E_INVALIDARG;
	}
	return launchTimestampRules( logits, rows, nVocab, tokenEot, tokenBeg, fedTokensDev, reset, (TimestampRecord*)recordsDev, (hipStream_t)stream );
}

int wh_op_boost_logits( void* stream, float* logits, int rows, int nVocab, int tokenEot, const int32_t* tablesDev, int64_t tableInts, const int32_t* fedTokensDev, int reset, int32_t* statesDev )
{
	if( !logits || !tablesDev || !statesDev || ( !reset && !fedTokensDev ) || rows < 1 || nVocab < 1 || nVocab > BOOST_MAX_VOCAB || tokenEot < 0 || tokenEot > nVocab ||
		tableInts < 4 || tableInts > BOOST_TABLE_INTS || reset < 0 || reset > 2 )
	{
		setError( "boost_logits: null pointer, empty shape, more than 65536 columns, eot outside the row, tables of fewer than 4 ints or a reset outside 0 .. 2" );
		return WH_E_INVALIDARG;
	}
	return launchBoostLogits( logits, rows, nVocab, tokenEot, tablesDev, (int)tableInts, fedTokensDev, reset, statesDev, (hipStream_t)stream );
}

int wh_op_no_repeat_ngram( void* stream, float* logits, int rows, int nVocab, int tokenEot, int n, const int32_t* fedDev, int reset, int32_t* historyDev, int32_t* countsDev, int cap )
{
	if( !logits || !historyDev || !countsDev || ( !reset && !fedDev ) || rows < 1 || nVocab < 1 || tokenEot < 0 || tokenEot > nVocab || n < 1 || n > NRN_MAX_N || reset < 0 || reset > 2 || cap < 1 )
	{
		setError( "no_repeat_ngram: null pointer, empty shape, eot outside the row, n outside 1 .. 8, a reset outside 0 .. 2 or a history without room" );
		return WH_E_INVALIDARG;
	}
	return launchNoRepeat( logits, rows, nVocab, tokenEot, n, fedDev, reset, historyDev, countsDev, cap, (hipStream_t)stream );
}

int wh_op_lang_probs( void* stream, const float* logits, int rows, int nVocab, int tokenSot, int nLang, float* langP, int32_t* best )
{
	if( !logits || !langP || !best || rows < 1 || nVocab < 1 || nVocab > 52224 || nLang < 1 || nLang > 1024 || tokenSot < 0 || (int64_t)tokenSot + 1 + nLang > nVocab )
	{
		setError( "lang_probs: bad pointer or size (at most 52224 columns), or the language block tokenSot + 1 .. tokenSot + nLang (1 .. 1024 tokens) leaves the row" );
		return WH_E_INVALIDARG;
	}
	return launchLangProbs( logits, nVocab, rows, nVocab, tokenSot, nLang, langP, best, (hipStream_t)stream );
}

int wh_op_token_scores( void* stream, const float* logits, int64_t rowStride, int rows, int nVocab, const int32_t* targetsDev, wh_token_score* outDev )
{
	static_assert( sizeof( wh_token_score ) == sizeof( TokenScore ) && sizeof( wh_token_score ) == 16, "token score layout" );
	if( !logits || !targetsDev || !outDev || rows < 1 || nVocab < 1 || rowStride < nVocab )
	{
		setError( "token_scores: null pointer, rows < 1, empty vocabulary or rowStride < nVocab" );
		return WH_E_INVALIDARG;
	}
	// the targets index the row on the device: checked here, before any launch
	std::vector<int32_t> t( (size_t)rows );
	WH_HIP( hipMemcpyAsync( t.data(), targetsDev, sizeof( int32_t ) * (size_t)rows, hipMemcpyDeviceToHost, (hipStream_t)stream ) );
	WH_HIP( hipStreamSynchronize( (hipStream_t)stream ) );
	for( int r = 0; r < rows; r++ )
		if( t[ (size_t)r ] < 0 || t[ (size_t)r ] >= nVocab )
		{
			setError( "token_scores: target " + std::to_string( t[ (size_t)r ] ) + " of row " + std::to_string( r ) + " is outside [0, " + std::to_string( nVocab ) + ")" );
			return WH_E_INVALIDARG;
		}
	return launchTokenScores( logits, rowStride, rows, nVocab, targetsDev, (TokenScore*)outDev, (hipStream_t)stream );
}

static bool tokenArgsOk(const float* probs, const wh_token_data* out, int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot )
{
	return probs && out && rows >= 1 && nVocab >= 1 && tokenBeg >= 1 && tokenBeg < nVocab && tokenSot >= 0 && tokenSot < tokenBeg && tokenSolm >= 0 &&
		tokenSolm < tokenBeg && tokenNot >= 0 && tokenNot < tokenBeg;
}

int wh_op_sample_best( void* stream, const float* probs, int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot,
	int forceTimestamp, int isInitial, wh_token_data* out )
{
	static_assert( sizeof( wh_token_data ) == sizeof( TokenData ), "token data layout" );
	if( !tokenArgsOk( probs, out, rows, nVocab, tokenBeg, tokenSot, tokenSolm, tokenNot ) ) { setError( "sample_best: bad pointer, size or token id" ); return WH_E_INVALIDARG; }
	return launchSampleBest( probs, rows, nVocab, tokenBeg, tokenSot, tokenSolm, tokenNot, forceTimestamp ? 1 : 0, isInitial ? 1 : 0, (TokenData*)out,
		(hipStream_t)stream );
}

int wh_op_vocab_soft_max_scaled( void* stream, const float* logits, float invT, float* probs, int rows, int cols )
{
	if( !logits || !probs || rows < 1 || cols < 1 ) { setError( "vocab_soft_max_scaled: null pointer or empty shape" ); return WH_E_INVALIDARG; }
	return launchVocabSoftMaxScaled( logits, invT, nullptr, probs, rows, cols, (hipStream_t)stream );
}

int wh_op_sample_draw( void* stream, const float* probs, int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot,
	int forceTimestamp, int isInitial, uint64_t seed, uint32_t nonce, const int32_t* positionsDev, wh_token_data* out )
{
	if( !tokenArgsOk( probs, out, rows, nVocab, tokenBeg, tokenSot, tokenSolm, tokenNot ) || !positionsDev || nVocab > SAMPLE_DRAW_MAX_VOCAB )
	{
		setError( "sample_draw: bad pointer, size (at most 65536 columns) or token id" );
		return WH_E_INVALIDARG;
	}
	return launchSampleDraw( probs, rows, nVocab, tokenBeg, tokenSot, tokenSolm, tokenNot, forceTimestamp ? 1 : 0, isInitial ? 1 : 0, seed, nonce, positionsDev,
		(TokenData*)out, (hipStream_t)stream );
}

// The per-row step outside a context: the records go to a temporary device array (the call waits for the stream at both ends: a test entry point)
int wh_op_sample_rows( void* stream, const float* logits, int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot, int forceTimestamp,
	int isInitial, const wh_sample_row* rowParams, const int32_t* positionsDev, float* probsOut, wh_token_data* out )
{
	if( !tokenArgsOk( logits, out, rows, nVocab, tokenBeg, tokenSot, tokenSolm, tokenNot ) || !rowParams || !positionsDev || !probsOut || nVocab > SAMPLE_DRAW_MAX_VOCAB )
	{
		setError( "sample_rows: bad pointer, size (at most 65536 columns) or token id" );
		return WH_E_INVALIDARG;
	}
	std::vector<SampleRowParams> host( (size_t)rows );
	for( int r = 0; r < rows; r++ )
	{
		const float t = rowParams[ r ].temperature;
		if( !( t >= 0.0f ) || t > 4.0f ) { setError( "sample_rows: a temperature lies outside [0, 4]" ); return WH_E_INVALIDARG; }
		host[ (size_t)r ] = makeSampleRow( t, rowParams[ r ].seed, rowParams[ r ].nonce );
	}
	hipStream_t st = (hipStream_t)stream;
	SampleRowParams* dev = nullptr;
	WH_HIP( hipMalloc( (void**)&dev, sizeof( SampleRowParams ) * (size_t)rows ) );
	const auto body = [ & ]() -> int
	{
		WH_HIP( hipMemcpyAsync( dev, host.data(), sizeof( SampleRowParams ) * (size_t)rows, hipMemcpyHostToDevice, st ) );
		WH_HIP( hipStreamSynchronize( st ) );
		WH_CHECK( launchVocabSoftMaxRows( logits, dev, probsOut, rows, nVocab, st ) );
		WH_CHECK( launchSampleRows( probsOut, rows, nVocab, tokenBeg, tokenSot, tokenSolm, tokenNot, forceTimestamp ? 1 : 0, isInitial ? 1 : 0, nullptr, dev, positionsDev,
			(TokenData*)out, nullptr, SampleMailbox{ nullptr, nullptr }, st ) );
		WH_HIP( hipStreamSynchronize( st ) );
		return 0;
	};
	const int rc = body();
	if( rc != 0 ) (void)hipStreamSynchronize( st );	   // whatever was launched has finished before the records go
	(void)hipFree( dev );
	return rc;
}

int wh_op_philox_u( void* stream, uint64_t seed, uint32_t nonce, int rows, const int32_t* positionsDev, double* uOut )
{
	if( rows < 1 || !positionsDev || !uOut ) { setError( "philox_u: null pointer or no rows" ); return WH_E_INVALIDARG; }
	return launchPhiloxU( seed, nonce, rows, positionsDev, uOut, (hipStream_t)stream );
}

int wh_op_beam_candidates( void* stream, const float* probs, int rows, int nVocab, int tokenBeg, int tokenSot, int tokenSolm, int tokenNot,
	int forceTimestamp, int isInitial, int width, wh_token_data* out )
{
	if( !tokenArgsOk( probs, out, rows, nVocab, tokenBeg, tokenSot, tokenSolm, tokenNot ) || width < 1 || width > 8 )
	{
		setError( "beam_candidates: bad pointer, size, token id or width (1 .. 8)" );
		return WH_E_INVALIDARG;
	}
	return launchBeamCandidates( probs, rows, nVocab, tokenBeg, tokenSot, tokenSolm, tokenNot, forceTimestamp ? 1 : 0, isInitial ? 1 : 0, width,
		(TokenData*)out, (hipStream_t)stream );
}

int wh_op_reorder_self_cache( void* stream, void* cacheK, void* cacheV, void* scratchK, void* scratchV, const int32_t* parents,
	const int32_t* rowsDev, int layers, int sequences, int maxSeq, int heads, int keyStride, int group )
{
	if( !cacheK || !cacheV || !scratchK || !scratchV || !parents || !rowsDev ) { setError( "reorder_self_cache: null pointer" ); return WH_E_INVALIDARG; }
	if( layers < 1 || sequences < 1 || sequences > maxSeq || heads < 1 || keyStride < 1 || group < 1 || group > sequences )
	{
		setError( "reorder_self_cache: need layers, heads, keyStride >= 1, 1 <= group <= sequences <= maxSeq" );
		return WH_E_INVALIDARG;
	}
	return launchReorderCacheDev( (f16*)cacheK, (f16*)cacheV, (f16*)scratchK, (f16*)scratchV, parents, rowsDev, layers, sequences, maxSeq, heads,
		keyStride, group, (hipStream_t)stream );
}


// ------------------------------------------------------------------------------------------------------------------
// micro-benchmarks used by tools/gemm_probe.py (development aid; not on the product path)
// ------------------------------------------------------------------------------------------------------------------
namespace
{
	// Grid-wide barrier cost probe: `n` rounds of { every workgroup publishes 64 bytes, barrier, reads another workgroup's
	// line and checks it }. One monotonic counter, agent-scope release on arrival, acquire polling, bounded spin.
	// mode 0: every workgroup polls the one counter; mode 1: arrivals are counted per XCD (workgroup id % 8) and the last
	// arrival of an XCD bumps the global counter by its XCD's population, so only 8 RMWs hit the shared line.
	__global__ void __launch_bounds__( 256 ) probeGridBarrier( unsigned* counters, float* buf, int n, int mode, int* err )
	{
		const unsigned G = gridDim.x, wg = blockIdx.x;
		const int lane = threadIdx.x;
		unsigned* const global = counters;
		unsigned* const perXcd = counters + 64 + ( wg & 7 ) * 64;	// own 256-byte line per counter
		const unsigned xcdPop = ( G + 7 - ( wg & 7 ) ) / 8;
		__shared__ int dead;
		if( lane == 0 ) dead = 0;
		for( int it = 0; it < n; it++ )
		{
			float* const slot = buf + ( it & 1 ) * G * 16;
			if( lane < 16 ) slot[ wg * 16 + lane ] = (float)( it * 7 + (int)wg + lane );
			__syncthreads();
			if( lane == 0 )
			{
				const unsigned target = (unsigned)( it + 1 ) * G;
				if( mode == 0 )
					__hip_atomic_fetch_add( global, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT );
				else
				{
					const unsigned prev = __hip_atomic_fetch_add( perXcd, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT );
					if( ( prev + 1 ) % xcdPop == 0 )
						__hip_atomic_fetch_add( global, xcdPop, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT );
				}
				unsigned spins = 0;
				while( __hip_atomic_load( global, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT ) < target )
				{
					if( ++spins > ( 1u << 21 ) )
					{
						*err = 2;
						dead = 1;
						break;
					}
				}
			}
			__syncthreads();
			if( dead ) return;
			const unsigned other = ( wg + 97 ) % G;
			if( lane < 16 )
			{
				const float got = __builtin_nontemporal_load( slot + other * 16 + lane );
				if( got != (float)( it * 7 + (int)other + lane ) ) *err = 1;
			}
		}
	}
	// max |a - b| over n floats (non-negative floats order like their bit patterns; NaN counts as +inf)
	__global__ void probeMaxDiff( const float* a, const float* b, long long n, int* out )
	{
		float m = 0.0f;
		for( long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x )
		{
			const float d = fabsf( a[ i ] - b[ i ] );
			m = ( d != d ) ? INFINITY : fmaxf( m, d );
		}
		for( int off = 32; off > 0; off >>= 1 ) m = fmaxf( m, __shfl_xor( m, off ) );
		if( ( threadIdx.x & 63 ) == 0 ) atomicMax( out, __float_as_int( m ) );
	}
	// logits-like FP32 values in [-6, 6)
	__global__ void probeFillF32( float* p, long long n, unsigned seed )
	{
		for( long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x )
		{
			unsigned h = (unsigned)i * 2654435761u + seed;
			h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
			p[ i ] = ( (float)( h & 0xFFFF ) / 32768.0f - 1.0f ) * 6.0f;
		}
	}
	__global__ void probeFill( _Float16* p, long long n, unsigned seed )
	{
		for( long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x )
		{
			unsigned h = (unsigned)i * 2654435761u + seed;
			h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
			p[ i ] = (_Float16)( ( (float)( h & 0xFFFF ) / 32768.0f - 1.0f ) * 0.5f );
		}
	}
}

int wh_debug_probe( wh_context* c, int kind, int variant, int M, int N, int K, int iters, float* msPerIter )
{
	if( !c || !msPerIter || iters <= 0 ) return WH_E_INVALIDARG;
	WH_BIND( c->m );
	hipStream_t st = c->stream;
	ProbeEvent e0, e1;
	ProbeMemory mem;
	WH_CHECK( e0.create() );
	WH_CHECK( e1.create() );
	int rc = 0;
	float ms = 0;
	if( kind == 0 || kind == 2 )
	{
		// chain of dependent empty kernels, `variant` workgroups of 256 threads each; kind 2 replays them from a graph
		const int grid = variant > 0 ? variant : 1;
		hipGraphExec_t exec = nullptr;
		const int perGraph = 100;
		if( kind == 2 )
		{
			hipGraph_t g = nullptr;
			WH_HIP( hipStreamBeginCapture( st, hipStreamCaptureModeThreadLocal ) );
			for( int i = 0; i < perGraph; i++ ) hipLaunchKernelGGL( probeEmpty, dim3( grid ), dim3( 256 ), 0, st, (int*)nullptr );
			WH_HIP( hipStreamEndCapture( st, &g ) );
			WH_HIP( hipGraphInstantiate( &exec, g, nullptr, nullptr, 0 ) );
			(void)hipGraphDestroy( g );
			WH_HIP( hipGraphLaunch( exec, st ) );
		}
		for( int i = 0; i < 20; i++ ) hipLaunchKernelGGL( probeEmpty, dim3( grid ), dim3( 256 ), 0, st, (int*)nullptr );
		WH_HIP( hipStreamSynchronize( st ) );
		WH_HIP( hipEventRecord( e0, st ) );
		if( kind == 2 )
			for( int i = 0; i < ( iters + perGraph - 1 ) / perGraph; i++ ) WH_HIP( hipGraphLaunch( exec, st ) );
		else
			for( int i = 0; i < iters; i++ ) hipLaunchKernelGGL( probeEmpty, dim3( grid ), dim3( 256 ), 0, st, (int*)nullptr );
		WH_HIP( hipEventRecord( e1, st ) );
		WH_HIP( hipEventSynchronize( e1 ) );
		WH_HIP( hipEventElapsedTime( &ms, e0, e1 ) );
		if( kind == 2 ) ms = ms * (float)iters / (float)( ( iters + perGraph - 1 ) / perGraph * perGraph );
		if( exec ) (void)hipGraphExecDestroy( exec );
	}
	else if( kind == 1 )
	{
		void *A = nullptr, *W = nullptr, *out = nullptr;
		WH_CHECK( mem.alloc( &A, (size_t)M * K * 2 ) );
		WH_CHECK( mem.alloc( &W, (size_t)N * K * 2 ) );
		WH_CHECK( mem.alloc( &out, (size_t)M * N * 4 ) );
		hipLaunchKernelGGL( probeFill, dim3( 1024 ), dim3( 256 ), 0, st, (_Float16*)A, (long long)M * K, 1u );
		hipLaunchKernelGGL( probeFill, dim3( 1024 ), dim3( 256 ), 0, st, (_Float16*)W, (long long)N * K, 2u );
		GemmArgs g = plainGemm( (const f16*)A, (const f16*)W, M, N, K );
		g.epi = EPI_F32; g.out32 = (float*)out;
		g.groupM = variant / 100;	   // variant = tile variant + 100 * M tiles per band of the block walk (0 = default)
		variant %= 100;
		unsigned long long* stamps = nullptr;
		if( variant == 35 || variant == 33 )
		{
			WH_CHECK( mem.alloc( &stamps, 32 ) );
			WH_HIP( hipMemsetAsync( stamps, 0, 32, st ) );
			g.pe = (const float*)stamps;
		}
		for( int i = 0; i < 2 && rc == 0; i++ ) rc = launchGemmVariant( g, variant, st );
		if( rc == 0 )
		{
			WH_HIP( hipStreamSynchronize( st ) );
			WH_HIP( hipEventRecord( e0, st ) );
			for( int i = 0; i < iters && rc == 0; i++ ) rc = launchGemmVariant( g, variant, st );
			WH_HIP( hipEventRecord( e1, st ) );
			WH_HIP( hipEventSynchronize( e1 ) );
			WH_HIP( hipEventElapsedTime( &ms, e0, e1 ) );
		}
		if( stamps && rc == 0 )
		{
			unsigned long long h[ 4 ] = {};
			WH_HIP( hipMemcpy( h, stamps, 32, hipMemcpyDeviceToHost ) );
			const double n = h[ 3 ] ? (double)h[ 3 ] : 1.0;
			fprintf( stderr, "[gemm8 stamps] %dx%dx%d: per tile (wave 0, cycles) first-operand wait %.0f, K loop %.0f, epilogue %.0f; %.0f tiles\n", M, N, K,
				h[ 0 ] / n, h[ 1 ] / n, h[ 2 ] / n, n );
		}
		// every variant is checked against the production path on the same operands: a pipeline that races is fast and wrong
		// (variants 31 .. 39 are ablations, wrong by construction)
		if( rc == 0 && ( variant == 34 || ( !( variant >= 31 && variant <= 39 ) && !( variant >= 41 && variant <= 49 ) && !( variant >= 60 && variant <= 69 ) ) ) )
		{
			void* ref = nullptr;
			int* diff = nullptr;
			WH_CHECK( mem.alloc( &ref, (size_t)M * N * 4 ) );
			WH_CHECK( mem.alloc( &diff, 4 ) );
			WH_HIP( hipMemsetAsync( diff, 0, 4, st ) );
			GemmArgs g2 = plainGemm( (const f16*)A, (const f16*)W, M, N, K );
			g2.epi = EPI_F32; g2.out32 = (float*)ref;
			static const int refVariant = []() { const char* e = getenv( "WH_PROBE_REF" ); return e ? atoi( e ) : 2; }();
			rc = launchGemmVariant( g2, refVariant, st );	   // 2 = the register-staged 128x128x32 kernel: shares no staging or scheduling code with the variants under test
			if( rc == 0 )
			{
				hipLaunchKernelGGL( probeMaxDiff, dim3( 2048 ), dim3( 256 ), 0, st, (const float*)out, (const float*)ref, (long long)M * N, diff );
				int bits = 0;
				WH_HIP( hipMemcpyAsync( &bits, diff, 4, hipMemcpyDeviceToHost, st ) );
				WH_HIP( hipStreamSynchronize( st ) );
				float md;
				memcpy( &md, &bits, 4 );
				if( getenv( "WH_PROBE_REF" ) ) fprintf( stderr, "[gemm probe] variant %d against variant %d, %d x %d x %d: max |diff| = %g\n", variant, refVariant, M, N, K, (double)md );
				if( !( md <= 1e-3f ) )
				{
					char buf[ 160 ];
					snprintf( buf, sizeof( buf ), "gemm probe: variant %d differs from the production kernel by %g", variant, (double)md );
					setError( buf );
					rc = -1;
				}
			}
		}
	}
	else if( kind == 3 )
	{
		// grid barrier: `variant` workgroups (must all be resident: <= number of CUs), M = mode, iters barriers per launch
		const int grid = variant > 0 ? variant : 256;
		unsigned* counters = nullptr;
		float* buf = nullptr;
		int* err = nullptr;
		WH_CHECK( mem.alloc( &counters, 4096 ) );
		WH_CHECK( mem.alloc( &buf, (size_t)grid * 16 * 2 * 4 ) );
		WH_CHECK( mem.alloc( &err, 4 ) );
		WH_HIP( hipMemsetAsync( err, 0, 4, st ) );
		for( int rep = 0; rep < 2; rep++ )
		{
			WH_HIP( hipMemsetAsync( counters, 0, 4096, st ) );
			WH_HIP( hipStreamSynchronize( st ) );
			WH_HIP( hipEventRecord( e0, st ) );
			hipLaunchKernelGGL( probeGridBarrier, dim3( grid ), dim3( 256 ), 0, st, counters, buf, iters, M, err );
			WH_HIP( hipEventRecord( e1, st ) );
			WH_HIP( hipEventSynchronize( e1 ) );
			WH_HIP( hipEventElapsedTime( &ms, e0, e1 ) );
		}
		int herr = 0;
		WH_HIP( hipMemcpy( &herr, err, 4, hipMemcpyDeviceToHost ) );
		if( herr != 0 )
		{
			setError( herr == 1 ? "grid barrier probe: stale data after the barrier" : "grid barrier probe: spin limit reached" );
			rc = -1;
		}
	}
	else if( kind == 4 )
	{
		// MFMA-bound product NEXT TO the HBM-bound cross-attention, measured directly: the encoder product of M x N x K (the production
		// launch: persistent gemmTiled8) `iters` times on stream A, attentionDecG<1,...> over `variant` windows x 16 heads x 1500 keys on stream B as often as fills
		// the same time; each alone, then together -- for the persistent grid limited to 256 / 224 / 192 / 160 / 128 CUs, without CU masks (the attention's
		// workgroups land where LDS and registers are free) and with complementary CU masks on the two streams. Results on stderr; ms = the unmasked 256-CU pair.
		const int wins = variant > 0 ? variant : 224, H = 16, T = 1500, d = H * HEAD_DIM;
		void *A = nullptr, *W = nullptr, *out = nullptr, *kc = nullptr, *vc = nullptr, *q = nullptr, *ao = nullptr;
		WH_CHECK( mem.alloc( &A, (size_t)M * K * 2 ) );
		WH_CHECK( mem.alloc( &W, (size_t)N * K * 2 ) );
		WH_CHECK( mem.alloc( &out, (size_t)M * N * 4 ) );
		const size_t kvBytes = (size_t)wins * H * T * HEAD_DIM * 2;
		WH_CHECK( mem.alloc( &kc, kvBytes ) );
		WH_CHECK( mem.alloc( &vc, kvBytes ) );
		WH_CHECK( mem.alloc( &q, (size_t)wins * d * 2 ) );
		WH_CHECK( mem.alloc( &ao, (size_t)wins * d * 2 ) );
		hipLaunchKernelGGL( probeFill, dim3( 1024 ), dim3( 256 ), 0, st, (_Float16*)A, (long long)M * K, 1u );
		hipLaunchKernelGGL( probeFill, dim3( 1024 ), dim3( 256 ), 0, st, (_Float16*)W, (long long)N * K, 2u );
		hipLaunchKernelGGL( probeFill, dim3( 1024 ), dim3( 256 ), 0, st, (_Float16*)kc, (long long)( kvBytes / 2 ), 3u );
		hipLaunchKernelGGL( probeFill, dim3( 1024 ), dim3( 256 ), 0, st, (_Float16*)vc, (long long)( kvBytes / 2 ), 4u );
		hipLaunchKernelGGL( probeFill, dim3( 1024 ), dim3( 256 ), 0, st, (_Float16*)q, (long long)wins * d, 5u );
		WH_HIP( hipStreamSynchronize( st ) );
		GemmArgs g = plainGemm( (const f16*)A, (const f16*)W, M, N, K );
		g.epi = EPI_F32; g.out32 = (float*)out;
		DecAttnArgs a = {};
		a.q = (const f16*)q; a.kc = (const f16*)kc; a.vc = (const f16*)vc; a.out = (f16*)ao;
		a.batch = wins; a.H = H; a.nTok = 1; a.nKeys = T; a.keyStride = T; a.causal = 0; a.group = 1;
		int cus = 0;
		WH_HIP( hipDeviceGetAttribute( &cus, hipDeviceAttributeMultiprocessorCount, c->m->device ) );
		auto wall = []() { return std::chrono::duration<double, std::milli>( std::chrono::steady_clock::now().time_since_epoch() ).count(); };
		auto timeIt = [ & ]( hipStream_t sa, hipStream_t sb, int nA, int nB, int cuLimit, double& msOut ) -> int
		{
			GemmArgs gl = g;
			gl.cuLimit = cuLimit;
			WH_HIP( hipDeviceSynchronize() );
			const double t0 = wall();
			// interleave the enqueues so that neither stream starts far ahead of the other
			const int n = std::max( nA, nB );
			for( int i = 0; i < n; i++ )
			{
				if( i < nA ) WH_CHECK( launchGemm( gl, sa ) );
				if( i < nB ) WH_CHECK( launchAttentionDec( a, sb ) );
			}
			WH_HIP( hipDeviceSynchronize() );
			msOut = wall() - t0;
			return 0;
		};
		hipStream_t sa = nullptr, sb = nullptr;
		WH_HIP( hipStreamCreateWithFlags( &sa, hipStreamNonBlocking ) );
		WH_HIP( hipStreamCreateWithFlags( &sb, hipStreamNonBlocking ) );
		double tA1 = 0, tB1 = 0, dummy = 0;
		rc = timeIt( sa, sb, 3, 3, 0, dummy );	   // warm-up
		if( rc == 0 ) rc = timeIt( sa, sb, iters, 0, 0, tA1 );
		if( rc == 0 ) rc = timeIt( sa, sb, 0, iters, 0, tB1 );
		const int nA = iters, nB = std::max( 1, (int)( iters * tA1 / std::max( tB1, 1e-6 ) + 0.5 ) );
		double tA = 0, tB = 0;
		if( rc == 0 ) rc = timeIt( sa, sb, nA, 0, 0, tA );
		if( rc == 0 ) rc = timeIt( sa, sb, 0, nB, 0, tB );
		if( rc == 0 )
		{
			fprintf( stderr, "[pair] product %d x %d x %d: %d launches %.2f ms alone (%.0f TFLOP/s); cross-attention %d windows: %d launches %.2f ms alone (%.2f TB/s)\n", M, N, K, nA, tA,
				2.0 * M * N * K * nA / tA * 1e-9, wins, nB, tB, 2.0 * kvBytes * nB / tB * 1e-9 );
			const int limits[] = { 0, 224, 192, 160, 128 };
			for( int li = 0; li < 5 && rc == 0; li++ )
			{
				const int lim = limits[ li ];
				double tAl = 0, tp = 0;
				rc = timeIt( sa, sb, nA, 0, lim, tAl );
				if( rc == 0 ) rc = timeIt( sa, sb, nA, nB, lim, tp );
				if( rc == 0 ) fprintf( stderr, "[pair] no masks, product on %3d CUs: product alone %.2f ms, pair %.2f ms = %.3f of (A + B) = %.3f of (A at this limit + B)\n", lim ? lim : cus, tAl, tp,
					tp / ( tA + tB ), tp / ( tAl + tB ) );
				if( li == 0 ) ms = (float)tp * (float)iters;
			}
			// complementary CU masks: CU i of the mask belongs to XCD i % 8 (a multiple of 8 keeps the split even over the XCDs)
			for( int li = 1; li < 5 && rc == 0; li++ )
			{
				const int lim = limits[ li ];
				uint32_t mA[ 16 ] = {}, mB[ 16 ] = {};
				const uint32_t words = (uint32_t)( ( cus + 31 ) / 32 );
				for( int i = 0; i < cus && i < 512; i++ ) ( i < lim ? mA : mB )[ i >> 5 ] |= 1u << ( i & 31 );
				hipStream_t ma = nullptr, mb = nullptr;
				if( hipExtStreamCreateWithCUMask( &ma, words, mA ) != hipSuccess || hipExtStreamCreateWithCUMask( &mb, words, mB ) != hipSuccess ) { fprintf( stderr, "[pair] CU-masked streams unavailable\n" ); break; }
				double tAl = 0, tBl = 0, tp = 0;
				rc = timeIt( ma, mb, nA, 0, lim, tAl );
				if( rc == 0 ) rc = timeIt( ma, mb, 0, nB, lim, tBl );
				if( rc == 0 ) rc = timeIt( ma, mb, nA, nB, lim, tp );
				if( rc == 0 ) fprintf( stderr, "[pair] masks %3d | %3d CUs: product alone %.2f ms, attention alone %.2f ms (%.2f TB/s), pair %.2f ms = %.3f of (A + B at 256 CUs)\n", lim, cus - lim, tAl, tBl,
					2.0 * kvBytes * nB / tBl * 1e-9, tp, tp / ( tA + tB ) );
				(void)hipStreamDestroy( ma ); (void)hipStreamDestroy( mb );
			}
		}
		(void)hipStreamDestroy( sa ); (void)hipStreamDestroy( sb );
	}
	else if( kind == 5 )
	{
		// The sampler of a decode step on M rows of N columns: variant 0 = the fused greedy sampler (launchSoftMaxSample), 1 = the per-row step with every row
		// greedy (launchVocabSoftMaxRows + launchSampleRows) -- what a round with one retrying row costs its greedy neighbours. The logits rotate through
		// buffers that together exceed the last-level cache (512 MB; at most 64 buffers); 5 warm-up launches, then the MEDIAN of `iters` launches, each between its
		// own events. Variant 2 = the logit filter of wh_context_set_suppress with K ids in front of the fused greedy sampler, 3 = the filter alone (tools/suppress_probe.py).
		// Variant 4 = the filter of wh_context_set_timestamp_rules in front of the fused greedy sampler, 5 = that filter alone (tools/timestamp_rules_probe.py); K is
		// the history the timed launch meets: 0 = text only, nothing masked; 1 = a closed pair, the timestamps masked (1501 columns); 2 = text then a timestamp, the
		// text tokens and the earlier timestamps masked (the widest mask; an untimed launch that feeds a text token goes in front of every timed one).
		// Variant 6 = the filter of wh_context_set_boost alone (tools/phrase_boost_probe.py); K is the set: 0 = one phrase of two tokens, 1 = 64 phrases, 2 = 1024
		// phrases of two tokens with 1024 distinct first tokens. Every row has just sampled the first token of phrase 0, so the timed launch searches the fed token,
		// boosts the node's offer and holds every root token against the node's table.
		// Variant 7 = the filter of wh_context_set_no_repeat with n = 3 in front of the fused greedy sampler, 8 = that filter alone (tools/no_repeat_probe.py); K is
		// the length of the history the timed launch masks by, 3 .. 448, the fed token included: tokens of a five-letter alphabet, so every lane's n-gram recurs and
		// stores. An untimed copy puts the counts back to K - 1 in front of every timed launch.
		const int rows = M, nVocab = N;
		if( rows < 1 || rows > 4096 || nVocab < 2048 || nVocab > 52224 || variant < 0 || variant > 8 ) return WH_E_INVALIDARG;
		const bool tsr = variant == 4 || variant == 5, boostOnly = variant == 6, nrn = variant == 7 || variant == 8;
		constexpr int nrnCap = 448, nrnN = 3;
		if( nrn && ( K < nrnN || K > nrnCap ) ) return WH_E_INVALIDARG;
		if( boostOnly && ( K < 0 || K > 2 ) ) return WH_E_INVALIDARG;
		if( tsr && ( K < 0 || K > 2 ) ) return WH_E_INVALIDARG;
		const int nIds = ( variant == 2 || variant == 3 ) ? K : 0;
		if( ( variant == 2 || variant == 3 ) && ( nIds < 1 || nIds > nVocab - 1607 ) ) return WH_E_INVALIDARG;
		const size_t rowBytes = (size_t)rows * nVocab * 4;
		const int nBuf = (int)std::min<size_t>( 64, ( (size_t)512 << 20 ) / rowBytes + 2 );
		std::vector<float*> logits( (size_t)nBuf, nullptr );
		float* probs = nullptr;
		DecodeState* state = nullptr;
		TokenData* out = nullptr;
		int *next = nullptr, *pos = nullptr;
		SampleRowParams* rowParams = nullptr;
		for( int b = 0; b < nBuf; b++ ) WH_CHECK( mem.alloc( &logits[ b ], rowBytes ) );
		WH_CHECK( mem.alloc( &probs, rowBytes ) );
		WH_CHECK( mem.alloc( &state, sizeof( DecodeState ) ) );
		WH_CHECK( mem.alloc( &out, sizeof( TokenData ) * (size_t)rows ) );
		WH_CHECK( mem.alloc( &next, sizeof( int ) * (size_t)rows ) );
		WH_CHECK( mem.alloc( &pos, sizeof( int ) * (size_t)rows ) );
		WH_CHECK( mem.alloc( &rowParams, sizeof( SampleRowParams ) * (size_t)rows ) );
		int* ids = nullptr;
		std::vector<int> idsHost( (size_t)nIds );
		// ascending ids spread over the text tokens, as a sorted set is
		for( int i = 0; i < nIds; i++ ) idsHost[ (size_t)i ] = (int)( (long long)i * ( nVocab - 1607 ) / nIds );
		if( nIds > 0 )
		{
			WH_CHECK( mem.alloc( &ids, sizeof( int ) * (size_t)nIds ) );
			WH_HIP( hipMemcpyAsync( ids, idsHost.data(), sizeof( int ) * (size_t)nIds, hipMemcpyHostToDevice, st ) );
		}
		for( int b = 0; b < nBuf; b++ ) hipLaunchKernelGGL( probeFillF32, dim3( 1024 ), dim3( 256 ), 0, st, logits[ b ], (long long)rows * nVocab, 11u + (unsigned)b );
		WH_HIP( hipMemsetAsync( state, 0, sizeof( DecodeState ), st ) );	 // step 0, no flags, no mailbox: every launch writes slot 0
		WH_HIP( hipMemsetAsync( pos, 0, sizeof( int ) * (size_t)rows, st ) );
		const std::vector<SampleRowParams> greedy( (size_t)rows, makeSampleRow( 0.0f, 0, 0 ) );
		WH_HIP( hipMemcpyAsync( rowParams, greedy.data(), sizeof( SampleRowParams ) * (size_t)rows, hipMemcpyHostToDevice, st ) );
		WH_HIP( hipStreamSynchronize( st ) );
		const int beg = nVocab - 1501, sot = beg - 105, solm = beg - 2, tnot = beg - 1;
		const SampleMailbox noMail = { nullptr, nullptr };
		int *fedText = nullptr, *fedTs = nullptr;
		TimestampRecord* records = nullptr;
		if( tsr )
		{
			WH_CHECK( mem.alloc( &fedText, sizeof( int ) * (size_t)rows ) );
			WH_CHECK( mem.alloc( &fedTs, sizeof( int ) * (size_t)rows ) );
			WH_CHECK( mem.alloc( &records, sizeof( TimestampRecord ) * (size_t)rows ) );
			const std::vector<int> text( (size_t)rows, 100 ), stamp( (size_t)rows, beg + 750 );
			WH_HIP( hipMemcpy( fedText, text.data(), sizeof( int ) * (size_t)rows, hipMemcpyHostToDevice ) );
			WH_HIP( hipMemcpy( fedTs, stamp.data(), sizeof( int ) * (size_t)rows, hipMemcpyHostToDevice ) );
			WH_CHECK( launchTimestampRules( probs, rows, nVocab, sot - 1, beg, nullptr, 1, records, st ) );
		}
		int *boostTab = nullptr, *boostStates = nullptr, *boostFed = nullptr;
		int boostInts = 0;
		if( boostOnly )
		{
			const int nPhrases = K == 0 ? 1 : K == 1 ? 64 : 1024;
			std::vector<int32_t> phr( (size_t)nPhrases * 2 ), lens( (size_t)nPhrases, 2 );
			for( int i = 0; i < nPhrases; i++ ) { phr[ (size_t)2 * i ] = 100 + 37 * i; phr[ (size_t)2 * i + 1 ] = 50 + i; }
			int64_t nInts = 0;
			WH_CHECK( wh_boost_compile( phr.data(), lens.data(), nPhrases, 2, sot - 1, nVocab, 2.5f, nullptr, 0, &nInts ) );
			std::vector<int32_t> tab( (size_t)nInts );
			WH_CHECK( wh_boost_compile( phr.data(), lens.data(), nPhrases, 2, sot - 1, nVocab, 2.5f, tab.data(), nInts, &nInts ) );
			boostInts = (int)nInts;
			WH_CHECK( mem.alloc( &boostTab, sizeof( int ) * (size_t)nInts ) );
			WH_CHECK( mem.alloc( &boostStates, sizeof( int ) * (size_t)rows ) );
			WH_CHECK( mem.alloc( &boostFed, sizeof( int ) * (size_t)rows ) );
			const std::vector<int> fedHost( (size_t)rows, phr[ 0 ] );
			WH_HIP( hipMemcpy( boostTab, tab.data(), sizeof( int ) * (size_t)nInts, hipMemcpyHostToDevice ) );
			WH_HIP( hipMemcpy( boostFed, fedHost.data(), sizeof( int ) * (size_t)rows, hipMemcpyHostToDevice ) );
			WH_CHECK( launchBoostLogits( probs, rows, nVocab, sot - 1, boostTab, boostInts, nullptr, 1, boostStates, st ) );
		}
		int *nrnHistory = nullptr, *nrnCounts = nullptr, *nrnCounts0 = nullptr, *nrnFed = nullptr;
		if( nrn )
		{
			WH_CHECK( mem.alloc( &nrnHistory, sizeof( int ) * (size_t)rows * nrnCap ) );
			WH_CHECK( mem.alloc( &nrnCounts, sizeof( int ) * (size_t)rows ) );
			WH_CHECK( mem.alloc( &nrnCounts0, sizeof( int ) * (size_t)rows ) );
			WH_CHECK( mem.alloc( &nrnFed, sizeof( int ) * (size_t)rows ) );
			std::vector<int> hist( (size_t)rows * nrnCap );
			for( size_t i = 0; i < hist.size(); i++ ) hist[ i ] = 100 + 37 * (int)( ( i % nrnCap ) % 5 );
			const std::vector<int> counts0( (size_t)rows, K - 1 ), fedHost( (size_t)rows, 100 + 37 * ( ( K - 1 ) % 5 ) );
			WH_HIP( hipMemcpy( nrnHistory, hist.data(), sizeof( int ) * hist.size(), hipMemcpyHostToDevice ) );
			WH_HIP( hipMemcpy( nrnCounts0, counts0.data(), sizeof( int ) * (size_t)rows, hipMemcpyHostToDevice ) );
			WH_HIP( hipMemcpy( nrnCounts, counts0.data(), sizeof( int ) * (size_t)rows, hipMemcpyHostToDevice ) );
			WH_HIP( hipMemcpy( nrnFed, fedHost.data(), sizeof( int ) * (size_t)rows, hipMemcpyHostToDevice ) );
		}
		const auto launch = [ & ]( float* x ) -> int
		{
			if( nrn )
			{
				WH_CHECK( launchNoRepeat( x, rows, nVocab, sot - 1, nrnN, nrnFed, 0, nrnHistory, nrnCounts, nrnCap, st ) );
				if( variant == 8 ) return 0;
				return launchSoftMaxSample( x, probs, rows, nVocab, beg, sot, solm, tnot, state, out, next, noMail, st );
			}
			if( boostOnly ) return launchBoostLogits( x, rows, nVocab, sot - 1, boostTab, boostInts, boostFed, 0, boostStates, st );
			if( tsr )
			{
				// K == 2: the untimed fold of a text token goes to the scratch row `probs`
				WH_CHECK( launchTimestampRules( x, rows, nVocab, sot - 1, beg, K == 0 ? fedText : fedTs, 0, records, st ) );
				if( variant == 5 ) return 0;
				return launchSoftMaxSample( x, probs, rows, nVocab, beg, sot, solm, tnot, state, out, next, noMail, st );
			}
			if( variant >= 2 ) WH_CHECK( launchSuppressLogits( x, rows, nVocab, ids, nullptr, nIds, nIds, st ) );
			if( variant == 3 ) return 0;
			if( variant == 0 || variant == 2 ) return launchSoftMaxSample( x, probs, rows, nVocab, beg, sot, solm, tnot, state, out, next, noMail, st );
			WH_CHECK( launchVocabSoftMaxRows( x, rowParams, probs, rows, nVocab, st ) );
			return launchSampleRows( probs, rows, nVocab, beg, sot, solm, tnot, 0, 0, state, rowParams, pos, out, next, noMail, st );
		};
		for( int i = 0; i < 5; i++ ) WH_CHECK( launch( logits[ (size_t)( i % nBuf ) ] ) );
		WH_HIP( hipStreamSynchronize( st ) );
		std::vector<float> each;
		for( int i = 0; i < iters; i++ )
		{
			if( tsr && K == 2 ) WH_CHECK( launchTimestampRules( probs, rows, nVocab, sot - 1, beg, fedText, 0, records, st ) );
			if( nrn ) WH_HIP( hipMemcpyAsync( nrnCounts, nrnCounts0, sizeof( int ) * (size_t)rows, hipMemcpyDeviceToDevice, st ) );
			WH_HIP( hipEventRecord( e0, st ) );
			WH_CHECK( launch( logits[ (size_t)( ( 5 + i ) % nBuf ) ] ) );
			WH_HIP( hipEventRecord( e1, st ) );
			WH_HIP( hipEventSynchronize( e1 ) );
			float t = 0;
			WH_HIP( hipEventElapsedTime( &t, e0, e1 ) );
			each.push_back( t );
		}
		std::sort( each.begin(), each.end() );
		ms = each[ each.size() / 2 ] * (float)iters;	  // (the caller gets ms / iters)
	}
	else
		rc = WH_E_INVALIDARG;
	*msPerIter = ms / (float)iters;
	return rc;
}

}	// extern "C"
