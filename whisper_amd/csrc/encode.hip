// The encoder graph (wh_encode*), the encoder gate and the profiled launch helpers the graphs share.
#include "runtime.h"

namespace wh
{
	std::mutex g_encGateMx;
	EncGate g_encGate[ 64 ];
}
int wh::gemmP( wh_context* c, const GemmArgs& g, bool skinny, bool decoder )
{
	const bool sk = skinny && g.M <= 32;
	const double flops = 2.0 * g.M * g.N * g.K;
	// algorithmic bytes: each operand once + the output once (FP16 in, 2..4 bytes out)
	const double bytes = 2.0 * g.N * g.K + 2.0 * g.M * g.K + ( g.out32 ? 4.0 : 2.0 ) * g.M * g.N;
	// a stream with a CU mask (WH_ENC_CUS): the persistent tiled kernel sizes its grid to the CUs it may use
	GemmArgs gl = g;
	if( c->encCus > 0 ) gl.cuLimit = c->stream == c->encStream ? c->encCus : c->totalCus - c->encCus;
	// Several contexts alive (batches in flight on their own streams): a workgroup of the persistent product owns its CU for the
	// whole launch (160 KiB of LDS, every register), so with all CUs taken a 10 us decode launch of the neighbouring batch waits up
	// to 2 ms for one. Leaving 4 CUs per XCD free costs the product 12 % of its CUs and returns 3 % of the whole job
	// (7389 -> 7627 audio-s/s, profiles/r03_ab_variants.txt); a lone context keeps the whole chip.
	else if( liveContexts( c->m ).load( std::memory_order_relaxed ) > 1 && c->totalCus >= 128 )
	{
		static const int spare = []() { const char* e = getenv( "WH_GEMM_SPARE_CUS" ); const int v = e ? atoi( e ) : 32; return v >= 0 && v <= 128 ? v & ~7 : 32; }();
		gl.cuLimit = c->totalCus - spare;
	}
	return profiled( c, sk ? KC_GEMM_SKINNY : ( decoder ? KC_GEMM_DEC : KC_GEMM_TILED ), flops, bytes, [ & ]() { return sk ? launchGemmSkinny( gl, c->stream ) : launchGemm( gl, c->stream ); } );
}
int wh::lnP( wh_context* c, const float* x, const float* w, const float* b, f16* out, int rows, int d, bool decoder )
{
	return profiled( c, decoder ? KC_LAYER_NORM_DEC : KC_LAYER_NORM, 8.0 * rows * d, 6.0 * rows * d, [ & ]() { return launchLayerNorm( x, w, b, out, rows, d, c->stream ); } );
}

// ------------------------------------------------------------------------------------------------------------------
// encoder
// ------------------------------------------------------------------------------------------------------------------
GemmArgs wh::plainGemm( const f16* A, const f16* W, int M, int N, int K )
{
	GemmArgs g;
	memset( &g, 0, sizeof( g ) );
	g.A = A; g.W = W; g.M = M; g.N = N; g.K = K;
	g.lda = K; g.Mb = M; g.aBatchStride = 0;
	g.ldc = N; g.cBatchStride = 0;
	g.scale = 1.0f;
	return g;
}

extern "C" {

static int encodeImpl( wh_context* c, const float* melDev, int batch, int64_t melLen, int64_t melStride, const int32_t* melOffsets, const wh_mel_window* wins = nullptr );

int wh_encode_windows( wh_context* c, const wh_mel_window* windows, int batch )
{
	if( !windows ) { setError( "encode_windows: windows is null" ); return WH_E_INVALIDARG; }
	return encodeImpl( c, nullptr, batch, 0, 0, nullptr, windows );
}

int wh_encode( wh_context* c, const float* melDev, int batch, int64_t melLen, int64_t melStride, const int32_t* melOffsets )
{
	if( !c || !c->encStream || c->prof.on ) return encodeImpl( c, melDev, batch, melLen, melStride, melOffsets );
	// everything queued so far (PCM upload, spectrogram) -> encoder on the low-priority stream -> the decode stream waits for it
	WH_BIND( c->m );
	WH_HIP( hipEventRecord( c->encReady, c->stream ) );
	WH_HIP( hipStreamWaitEvent( c->encStream, c->encReady, 0 ) );
	hipStream_t const main = c->stream;
	c->stream = c->encStream;
	const int rc = encodeImpl( c, melDev, batch, melLen, melStride, melOffsets );
	c->stream = main;
	WH_CHECK( rc );
	WH_HIP( hipEventRecord( c->encDone, c->encStream ) );
	WH_HIP( hipStreamWaitEvent( c->stream, c->encDone, 0 ) );
	return 0;
}

static int encodeImpl( wh_context* c, const float* melDev, int batch, int64_t melLen, int64_t melStride, const int32_t* melOffsets, const wh_mel_window* wins )
{
	if( !c || ( !melDev && !wins ) || batch <= 0 || batch > c->maxBatch || ( !wins && melLen <= 0 ) ) { setError( "encode: bad argument" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	const wh_model* m = c->m;
	const wh_hparams& hp = m->hp;
	const Layout& L = m->L;
	hipStream_t st = c->stream;
	const int d = hp.n_audio_state, H = hp.n_audio_head, T = c->T;
	const int batchAll = batch;

	if( batch > wh_context::PIN_WINDOWS ) { setError( "encode: batch too large" ); return WH_E_INVALIDARG; }
	if( c->flags & WH_FLAG_PARITY_EXACT ) return encodeExact( c, melDev, batch, melLen, melStride, melOffsets, wins );
	if( batch > c->encChunk && ( c->flags & WH_FLAG_DEBUG_CAPTURE ) ) { setError( "encode: the probe-point capture needs a batch of one encoder chunk" ); return WH_E_INVALIDARG; }
	const bool gated = ( g_tuning & TUNE_ENC_SERIAL ) && batch >= ENC_SERIAL_MIN_WINDOWS && liveContexts( m ).load( std::memory_order_relaxed ) > 1;
	if( gated )
	{
		std::lock_guard<std::mutex> lk( g_encGateMx );
		EncGate& gate = g_encGate[ m->device & 63 ];
		if( gate.last && gate.owner != c ) WH_HIP( hipStreamWaitEvent( st, gate.last, 0 ) );
	}
	// offsets go through pinned staging (ints [0, 4096)): the copy is truly asynchronous and the call never blocks.
	// The staging is rewritten by the next wh_encode only, which the stream orders after this copy has been consumed
	// as long as the caller synchronises once per window (wh_decode / wh_decode_window_finish do).
	const MelWindow* winsDev = nullptr;
	if( wins )
	{
		// per-window sources (wh_encode_windows): descriptors through the same staging, 6 ints each
		static_assert( sizeof( MelWindow ) == 24 && sizeof( wh_mel_window ) == 24, "window descriptor layout" );
		if( (size_t)batch * sizeof( MelWindow ) > wh_context::PIN_WINDOWS * sizeof( int32_t ) ) { setError( "encode_windows: batch too large" ); return WH_E_INVALIDARG; }
		MelWindow* const stage = (MelWindow*)c->pinned;
		for( int i = 0; i < batch; i++ )
		{
			if( wins[ i ].melDev && ( wins[ i ].melLen <= 0 || wins[ i ].offset < 0 ) ) { setError( "encode_windows: bad window" ); return WH_E_INVALIDARG; }
			stage[ i ] = MelWindow{ wins[ i ].melDev, (long long)wins[ i ].melLen, wins[ i ].offset, 0 };
		}
		WH_HIP( hipMemcpyAsync( c->melWindowsDev, stage, sizeof( MelWindow ) * batch, hipMemcpyHostToDevice, st ) );
		winsDev = c->melWindowsDev;
	}
	else
	{
		for( int i = 0; i < batch; i++ ) c->pinned[ i ] = melOffsets ? melOffsets[ i ] : 0;
		WH_HIP( hipMemcpyAsync( c->melOffsetsDev, c->pinned, sizeof( int32_t ) * batch, hipMemcpyHostToDevice, st ) );
	}
	// A batch larger than the encoder's chunk is encoded chunk by chunk through the same activations: windows are independent, the
	// products are MFMA-bound and saturated at a chunk's row count, and only the cross-attention caches (written in place at the
	// chunk's window offset) are sized for the whole batch.
	const int nChunks = ( batchAll + c->encChunk - 1 ) / c->encChunk;
	const int perChunk = ( batchAll + nChunks - 1 ) / nChunks;
	for( int b0 = 0; b0 < batchAll; b0 += perChunk )
	{
	batch = std::min( perChunk, batchAll - b0 );
	const int M = batch * T;
	WH_CHECK( profiled( c, KC_MEL_TO_CONV, 0.0, 6.0 * batch * 2.0 * T * hp.n_mels,
		[ & ]() { return launchMelToConvInput( melDev ? melDev + (int64_t)b0 * melStride : nullptr, melStride, melLen, c->melOffsetsDev + b0, winsDev ? winsDev + b0 : nullptr,
			c->convIn, c->convInStride, hp.n_mels, 2 * T, batch, st ); } ) );

	// conv1 (k=3, stride 1, pad 1) + bias + GELU as an implicit GEMM over the padded time-major input:
	// row t of the im2col matrix is the contiguous slice starting at padded row t (whisper.cpp:1127-1136; ggml.c:5199-5318)
	{
		GemmArgs g = plainGemm( c->convIn, m->at<f16>( L.conv1w ), batch * 2 * T, d, conv1Kpad( hp ) );
		g.lda = hp.n_mels; g.Mb = 2 * T; g.aBatchStride = c->convInStride;
		g.epi = EPI_F16_GELU;
		g.bias = m->at<float>( L.conv1b );
		g.out16 = c->conv1Out + d;	 // padded row t+1
		g.ldc = d; g.cBatchStride = c->conv1Stride;
		WH_CHECK( gemmP( c, g, false ) );
	}
	WH_CHECK( capture( c, c->capTemp1, c->conv1Out, (int64_t)batch * c->conv1Stride, (int64_t)c->maxBatch * c->conv1Stride ) );	// "enc.temp1"
	// conv2 (stride 2) + bias + GELU + positional embedding -> residual stream x [batch*T][d] (whisper.cpp:1138-1167)
	{
		GemmArgs g = plainGemm( c->conv1Out, m->at<f16>( L.conv2w ), M, d, 3 * d );
		g.lda = 2 * d; g.Mb = T; g.aBatchStride = c->conv1Stride;
		g.epi = EPI_CONV2;
		g.bias = m->at<float>( L.conv2b );
		g.pe = m->at<float>( L.encPe );
		g.out32 = c->x; g.ldc = d;
		WH_CHECK( gemmP( c, g, false ) );
	}
	WH_CHECK( capture( c, c->capLayer0In, c->x, (int64_t)M * d, (int64_t)c->maxBatch * T * d ) );	// "enc.layer[ 0 ].in"
	for( int il = 0; il < hp.n_audio_layer; il++ )
	{
		const EncLayer& e = L.enc[ il ];
		WH_CHECK( lnP( c, c->x, m->at<float>( e.ln1w ), m->at<float>( e.ln1b ), c->xn, M, d ) );
		{
			GemmArgs g = plainGemm( c->xn, m->at<f16>( e.wqkv ), M, 3 * d, d );
			g.epi = EPI_QKV_ENC;
			g.bias = m->at<float>( e.bqkv );
			g.q = c->q; g.k = c->k; g.v = c->vT;
			g.T = T; g.Tpad = c->Tpad; g.H = H; g.B = batch;
			WH_CHECK( gemmP( c, g, false ) );
		}
		WH_CHECK( profiled( c, KC_ATTN_ENC, 4.0 * batch * H * (double)T * T * HEAD_DIM, 2.0 * 4.0 * batch * H * (double)T * HEAD_DIM,
			[ & ]() { return launchAttentionEnc( c->q, c->k, c->vT, c->attn, batch, H, T, c->Tpad, ( c->flags & WH_FLAG_PARITY_PV ) != 0, m->at<f16>( L.expTab ), st ); } ) );
		if( il == 0 ) WH_CHECK( capture( c, c->capEncKqv, c->attn, (int64_t)M * d, (int64_t)c->maxBatch * T * d ) );	// "enc-KQV"
		{
			GemmArgs g = plainGemm( c->attn, m->at<f16>( e.wo ), M, d, d );
			g.epi = EPI_F32;
			g.bias = m->at<float>( e.bo );
			g.res = c->x; g.out32 = c->x;
			WH_CHECK( gemmP( c, g, false ) );
		}
		WH_CHECK( lnP( c, c->x, m->at<float>( e.ln2w ), m->at<float>( e.ln2b ), c->xn, M, d ) );
		{
			GemmArgs g = plainGemm( c->xn, m->at<f16>( e.w1 ), M, 4 * d, d );
			g.epi = EPI_F16_GELU;
			g.bias = m->at<float>( e.b1 );
			g.out16 = c->h;
			WH_CHECK( gemmP( c, g, false ) );
		}
		{
			GemmArgs g = plainGemm( c->h, m->at<f16>( e.w2 ), M, d, 4 * d );
			g.epi = EPI_F32;
			g.bias = m->at<float>( e.b2 );
			g.res = c->x; g.out32 = c->x;
			WH_CHECK( gemmP( c, g, false ) );
		}
	}
	WH_CHECK( lnP( c, c->x, m->at<float>( L.lnPostW ), m->at<float>( L.lnPostB ), c->xn, M, d ) );
	// cross-attention K/V of every decoder layer in one product (whisper.cpp:1448-1487)
	{
		GemmArgs g = plainGemm( c->xn, m->at<f16>( L.wcross ), M, 2 * hp.n_text_layer * d, d );
		g.epi = EPI_CROSS_KV;
		g.bias = m->at<float>( L.bcross );
		g.scale = (float)pow( (double)( (float)d / (float)H ), -0.25 );
		// [layer][window][head][T][64]: the chunk's first window; the layer stride stays maxBatch windows
		g.k = c->crossK + (int64_t)b0 * T * d; g.v = c->crossV + (int64_t)b0 * T * d;
		g.T = T; g.H = H; g.B = c->maxBatch;
		WH_CHECK( gemmP( c, g, false ) );
	}
	}	// chunks
	batch = batchAll;
	if( gated )
	{
		std::lock_guard<std::mutex> lk( g_encGateMx );
		if( !c->encGateEv ) WH_HIP( hipEventCreateWithFlags( &c->encGateEv, hipEventDisableTiming ) );
		WH_HIP( hipEventRecord( c->encGateEv, st ) );
		EncGate& gate = g_encGate[ m->device & 63 ];
		gate.last = c->encGateEv;
		gate.owner = c;
	}
	c->encoded = true;
	c->lastEncBatch = batch;
	c->lastBatch = batch * c->hyp;
	return 0;
}

}	// extern "C"
