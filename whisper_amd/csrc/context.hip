// The context: creation and its buffers, the owner of device memory, plain device buffers, the mel entry points.
#include "runtime.h"

namespace wh
{
	std::atomic<int> g_liveContextsDev[ 64 ];

	hipError_t guardedAlloc( Allocation& a, int64_t bytes, int fill, const char* name, hipStream_t stream )
	{
		void* v = nullptr;
		const int64_t guard = wh_context::debugGuardBytes();
		hipError_t e = hipMalloc( &v, (size_t)( bytes + 2 * guard ) );
		if( e != hipSuccess ) return e;
		uint8_t* const body = (uint8_t*)v + guard;
		if( guard )
		{
			e = hipMemsetAsync( v, wh_context::GUARD_BYTE, (size_t)guard, stream );
			if( e == hipSuccess ) e = hipMemsetAsync( body + bytes, wh_context::GUARD_BYTE, (size_t)guard, stream );
		}
		if( e == hipSuccess && fill >= 0 ) e = hipMemsetAsync( body, fill, (size_t)bytes, stream );
		if( e != hipSuccess ) { (void)hipFree( v ); return e; }
		a = { v, body, bytes, name };
		return hipSuccess;
	}

	int guardedFree( const Allocation& a )
	{
		int bad = 0;
		if( const int64_t guard = (int64_t)( (const uint8_t*)a.body - (const uint8_t*)a.base ) )
		{
			std::vector<uint8_t> h( (size_t)guard );
			for( int side = 0; side < 2; side++ )
			{
				const uint8_t* const src = side ? (const uint8_t*)a.body + a.bytes : (const uint8_t*)a.base;
				if( hipMemcpy( h.data(), src, (size_t)guard, hipMemcpyDeviceToHost ) != hipSuccess ) continue;
				for( int64_t i = 0; i < guard; i++ )
					if( h[ (size_t)i ] != wh_context::GUARD_BYTE )
					{
						const long long offset = (long long)( side ? a.bytes + i : i - guard );
						if( a.name ) fprintf( stderr, "WH_GUARD_VIOLATION: buffer '%s' (%lld bytes): write at offset %lld\n", a.name, (long long)a.bytes, offset );
						else fprintf( stderr, "WH_GUARD_VIOLATION: wh_buffer_alloc buffer (%lld bytes): write at offset %lld\n", (long long)a.bytes, offset );
						bad++;
						break;
					}
			}
		}
		const hipError_t e = hipFree( a.base );
		return e == hipSuccess ? bad : hipFail( e, "hipFree", __FILE__, __LINE__ );
	}
}
namespace
{
	constexpr int MEL_BATCH_MAX = 1024;	   // buffers per launch of wh_mel_spectrogram_batch (a maximum each in the context's scratch)
}

extern "C" {

// ==================================================================================================================
// context
// ==================================================================================================================
int wh_context_create( wh_model* m, int maxBatch, void* stream, wh_context** out )
{
	return wh_context_create_hyp( m, maxBatch, 1, stream, out );
}

int wh_context_create_hyp( wh_model* m, int maxBatch, int hypotheses, void* stream, wh_context** out )
{
	if( !m || !out || maxBatch <= 0 || hypotheses <= 0 || hypotheses > 8 || hypotheses == 6 || hypotheses == 7 )
	{
		setError( "context_create: bad argument (hypotheses per window: 1, 2, 3, 4, 5 or 8)" );
		return WH_E_INVALIDARG;
	}
	if( !m->finalized ) { setError( "context_create: model is not finalized" ); return WH_E_NOT_READY; }
	WH_BIND( m );
	wh_context* c = new wh_context();
	liveContexts( m ).fetch_add( 1 );
	c->m = m;
	(void)hipDeviceGetAttribute( &c->totalCus, hipDeviceAttributeMultiprocessorCount, m->device );
	c->maxBatch = maxBatch;
	c->hyp = hypotheses;
	c->maxSeq = maxBatch * hypotheses;
	c->stream = (hipStream_t)stream;
	if( !c->stream )
	{
		// the legacy null stream cannot be captured into a hipGraph: own a non-blocking stream instead
		hipError_t e;
		if( g_tuning & TUNE_SPLIT_STREAMS )
		{
			int lo = 0, hi = 0;
			(void)hipDeviceGetStreamPriorityRange( &lo, &hi );	   // lo = least, hi = greatest priority (numerically lower)
			// WH_ENC_CUS = n: SPATIAL split instead of priorities -- the encoder stream may use n CUs, the decode stream the others.
			// The persistent encoder GEMM takes a whole CU (160 KiB of LDS, every register), so two batches in flight otherwise
			// take turns; with disjoint CU sets the MFMA-bound encoder of one batch runs beside the HBM-bound decode chain of the
			// other. Mask bit i is a CU of XCD i % 8 (the driver spreads a queue's mask over the XCDs), so the low n bits give the
			// encoder n / 8 CUs of EVERY XCD and both sides keep all eight L2s and fabric links.
			int encCus = 0, cus = 0;
			if( const char* ev = getenv( "WH_ENC_CUS" ) ) encCus = atoi( ev );
			(void)hipDeviceGetAttribute( &cus, hipDeviceAttributeMultiprocessorCount, m->device );
			if( encCus >= 8 && encCus <= cus - 8 )
			{
				encCus &= ~7;
				uint32_t maskE[ 16 ] = {}, maskD[ 16 ] = {};
				for( int i = 0; i < cus && i < 512; i++ ) ( i < encCus ? maskE : maskD )[ i >> 5 ] |= 1u << ( i & 31 );
				const uint32_t words = (uint32_t)( ( cus + 31 ) / 32 );
				e = hipExtStreamCreateWithCUMask( &c->stream, words, maskD );
				if( e == hipSuccess ) e = hipExtStreamCreateWithCUMask( &c->encStream, words, maskE );
				c->encCus = encCus;
				c->totalCus = cus;
			}
			else
			{
				e = hipStreamCreateWithPriority( &c->stream, hipStreamNonBlocking, hi );
				if( e == hipSuccess ) e = hipStreamCreateWithPriority( &c->encStream, hipStreamNonBlocking, lo );
			}
			if( e == hipSuccess ) e = hipEventCreateWithFlags( &c->encReady, hipEventDisableTiming );
			if( e == hipSuccess ) e = hipEventCreateWithFlags( &c->encDone, hipEventDisableTiming );
		}
		else
			e = hipStreamCreateWithFlags( &c->stream, hipStreamNonBlocking );
		c->ownsStream = true;
		if( e != hipSuccess ) { wh_context_destroy( c ); return hipFail( e, "hipStreamCreate", __FILE__, __LINE__ ); }	// releases whichever streams / events exist
	}
	const wh_hparams& hp = m->hp;
	const int64_t d = hp.n_audio_state, B = maxBatch, H = hp.n_audio_head, S = c->maxSeq;
	const int T = hp.n_audio_ctx;
	c->T = T;
	c->Tpad = roundUp( T, 256 );
	c->maxRows = c->maxSeq * hp.n_text_ctx;
	{
		// option enc_chunk = the most windows one encoder pass takes (default 128); a larger batch is cut into equal chunks
		const int chunkMax = g_opt.encChunk >= 1 && g_opt.encChunk <= 1024 ? g_opt.encChunk : 128;
		const int nChunks = ( maxBatch + chunkMax - 1 ) / chunkMax;
		c->encChunk = ( maxBatch + nChunks - 1 ) / nChunks;
	}
	const int64_t Be = c->encChunk;
	const int64_t rowsE = Be * T;
	c->convInStride = ( 2ll * T + 2 ) * hp.n_mels;
	c->conv1Stride = ( 2ll * T + 2 ) * d;
	int rc = 0;
	// conv1 is an implicit GEMM whose row t is the K = conv1Kpad halfs starting at padded row t (stride n_mels): the last
	// row of the last window therefore reads conv1Kpad - 3 n_mels halfs (16 at 80 mels, 0 at 128) past the logical end. Those
	// columns meet zero weights (the padded part of conv1w's rows), but the operand must still be finite: the tail is part
	// of the allocation and, like the padding rows, stays zero for the life of the context. conv2 (K = 3 d over rows of
	// stride 2 d, last row ending at (2 T + 1) d) never leaves its (2 T + 2) d rows.
	const int64_t conv1Tail = conv1Kpad( hp ) - 3 * hp.n_mels;
	rc = rc ? rc : c->alloc( c->convIn, Be * c->convInStride + conv1Tail, wh_context::MUST_BE_ZERO, "convIn" );
	rc = rc ? rc : c->alloc( c->conv1Out, Be * c->conv1Stride, wh_context::MUST_BE_ZERO, "conv1Out" );
	rc = rc ? rc : c->alloc( c->x, rowsE * d, wh_context::DONT_CARE, "x" );
	rc = rc ? rc : c->alloc( c->xn, rowsE * d, wh_context::DONT_CARE, "xn" );
	rc = rc ? rc : c->alloc( c->q, rowsE * d, wh_context::DONT_CARE, "q" );
	rc = rc ? rc : c->alloc( c->k, rowsE * d, wh_context::DONT_CARE, "k" );
	rc = rc ? rc : c->alloc( c->vT, Be * H * HEAD_DIM * c->Tpad, wh_context::MUST_BE_ZERO, "vT" );
	rc = rc ? rc : c->alloc( c->attn, rowsE * d, wh_context::DONT_CARE, "attn" );
	rc = rc ? rc : c->alloc( c->h, rowsE * 4 * d, wh_context::DONT_CARE, "h" );
	rc = rc ? rc : c->alloc( c->crossK, (int64_t)hp.n_text_layer * B * T * d, wh_context::MUST_BE_ZERO, "crossK" );
	rc = rc ? rc : c->alloc( c->crossV, (int64_t)hp.n_text_layer * B * T * d, wh_context::MUST_BE_ZERO, "crossV" );
	rc = rc ? rc : c->alloc( c->selfK, (int64_t)hp.n_text_layer * S * hp.n_text_ctx * d, wh_context::MUST_BE_ZERO, "selfK" );
	rc = rc ? rc : c->alloc( c->selfV, (int64_t)hp.n_text_layer * S * hp.n_text_ctx * d, wh_context::MUST_BE_ZERO, "selfV" );
	const int64_t rowsD = c->maxRows;
	rc = rc ? rc : c->alloc( c->dx, rowsD * d, wh_context::DONT_CARE, "dx" );
	rc = rc ? rc : c->alloc( c->dxn, rowsD * d, wh_context::DONT_CARE, "dxn" );
	rc = rc ? rc : c->alloc( c->dq, rowsD * d, wh_context::DONT_CARE, "dq" );
	rc = rc ? rc : c->alloc( c->dattn, rowsD * d, wh_context::DONT_CARE, "dattn" );
	rc = rc ? rc : c->alloc( c->dh, rowsD * 4 * d, wh_context::DONT_CARE, "dh" );
	rc = rc ? rc : c->alloc( c->splitK, 8ll * ( rowsD < GEMV_FUSED_MAX_ROWS ? rowsD : GEMV_FUSED_MAX_ROWS ) * d, wh_context::DONT_CARE, "splitK" );	   // partial tiles of the K-split MLP down-projection (33 .. 128 rows)
	{
		const int64_t sm = S < SMALL_MAX_ROWS ? S : SMALL_MAX_ROWS;
		rc = rc ? rc : c->alloc( c->crossScores, sm * hp.n_text_head * T, wh_context::DONT_CARE, "crossScores" );
		rc = rc ? rc : c->alloc( c->crossSplitMax, sm * hp.n_text_head * CROSS_SPLITS, wh_context::DONT_CARE, "crossSplitMax" );
		rc = rc ? rc : c->alloc( c->crossPart, sm * hp.n_text_head * CROSS_SPLITS * CROSS_PART, wh_context::DONT_CARE, "crossPart" );
	}
	rc = rc ? rc : c->alloc( c->logits, S * (int64_t)hp.n_vocab, wh_context::DONT_CARE, "logits" );
	rc = rc ? rc : c->alloc( c->probs, S * (int64_t)hp.n_vocab, wh_context::DONT_CARE, "probs" );
	rc = rc ? rc : c->alloc( c->tokensDev, rowsD, wh_context::DONT_CARE, "tokensDev" );
	rc = rc ? rc : c->alloc( c->melOffsetsDev, B, wh_context::DONT_CARE, "melOffsetsDev" );
	rc = rc ? rc : c->alloc( c->melWindowsDev, B, wh_context::MUST_BE_ZERO, "melWindowsDev" );
	rc = rc ? rc : c->alloc( c->tokDataDev, S, wh_context::DONT_CARE, "tokDataDev" );
	rc = rc ? rc : c->alloc( c->melScratch, 64 + 4 * MEL_BATCH_MAX, wh_context::DONT_CARE, "melScratch" );	  // [0..15]: the single / streamed entry points, then one maximum per buffer of a batch
	rc = rc ? rc : c->alloc( c->state, 1, wh_context::MUST_BE_ZERO, "state" );
	rc = rc ? rc : c->alloc( c->seqPos, S, wh_context::MUST_BE_ZERO, "seqPos" );
	if( rc == 0 )
	{
		c->pinnedInts = wh_context::PIN_POS + S + S * (int64_t)hp.n_text_ctx;
		const hipError_t e = hipHostMalloc( (void**)&c->pinned, sizeof( int32_t ) * (size_t)c->pinnedInts, hipHostMallocDefault );
		if( e != hipSuccess ) rc = hipFail( e, "hipHostMalloc", __FILE__, __LINE__ );
	}
	rc = rc ? rc : c->alloc( c->greedyOut, (int64_t)hp.n_text_ctx * S, wh_context::DONT_CARE, "greedyOut" );
	if( rc == 0 && !getenv( "WH_NO_MAILBOX" ) )
	{
		// optional: without it (allocation refused, WH_NO_MAILBOX) wh_decode_window_fetch waits for an event and copies
		const size_t n = (size_t)hp.n_text_ctx * S;
		void *d = nullptr, *f = nullptr;
		if( hipHostMalloc( &d, n * sizeof( TokenData ), hipHostMallocMapped | hipHostMallocCoherent ) == hipSuccess &&
			hipHostMalloc( &f, 2 * n * sizeof( int ), hipHostMallocMapped | hipHostMallocCoherent ) == hipSuccess )
		{
			memset( f, 0, 2 * n * sizeof( int ) );	   // stamp + checksum per record
			void *dd = nullptr, *fd = nullptr;
			if( hipHostGetDevicePointer( &dd, d, 0 ) == hipSuccess && hipHostGetDevicePointer( &fd, f, 0 ) == hipSuccess )
			{
				c->mailData = (TokenData*)d; c->mailFlag = (int*)f;
				c->mailDev = { (TokenData*)dd, (int*)fd };
				d = f = nullptr;
			}
		}
		if( d ) (void)hipHostFree( d );
		if( f ) (void)hipHostFree( f );
		(void)hipGetLastError();
	}
	if( rc == 0 )
	{
		const hipError_t e = hipStreamSynchronize( c->stream );
		if( e != hipSuccess ) rc = hipFail( e, "hipStreamSynchronize", __FILE__, __LINE__ );
	}
	if( rc != 0 )
	{
		wh_context_destroy( c );
		return rc;
	}
	*out = c;
	return 0;
}

void wh_context_destroy( wh_context* c )
{
	if( !c ) return;
	liveContexts( c->m ).fetch_sub( 1 );
	(void)bindDevice( c->m );
	if( c->stream ) (void)hipStreamSynchronize( c->stream );
	c->destroyStepGraphs();
	for( auto& mk : c->marks ) (void)hipEventDestroy( mk.ev );
	for( hipEvent_t e : c->markPool ) (void)hipEventDestroy( e );
	if( c->copyStream ) (void)hipStreamDestroy( c->copyStream );
	if( c->encStream ) { (void)hipStreamSynchronize( c->encStream ); (void)hipStreamDestroy( c->encStream ); }
	if( c->encReady ) (void)hipEventDestroy( c->encReady );
	if( c->encDone ) (void)hipEventDestroy( c->encDone );
	{
		std::lock_guard<std::mutex> lk( g_encGateMx );
		for( EncGate& gate : g_encGate )
			if( gate.owner == c ) gate = EncGate{};
	}
	if( c->encGateEv ) (void)hipEventDestroy( c->encGateEv );
	if( c->noSpeechEv ) (void)hipEventDestroy( c->noSpeechEv );
	if( c->sampleRowsEv ) (void)hipEventDestroy( c->sampleRowsEv );
	if( c->sampleRowsPin ) (void)hipHostFree( c->sampleRowsPin );
	int bad = 0;
	for( const Allocation& a : c->allocations ) bad += guardedFree( a ) > 0;
	if( bad != 0 ) fprintf( stderr, "WH_GUARD_VIOLATION: context %p wrote outside its buffers\n", (void*)c );
	if( c->pinned ) (void)hipHostFree( c->pinned );
	if( c->mailData ) (void)hipHostFree( c->mailData );
	if( c->mailFlag ) (void)hipHostFree( c->mailFlag );
	if( c->ownsStream && c->stream ) (void)hipStreamDestroy( c->stream );
	delete c;
}

int wh_context_bind( wh_context* c )
{
	if( !c ) return WH_E_INVALIDARG;
	WH_BIND( c->m );
	return 0;
}

int wh_context_set_audio_ctx( wh_context* c, int audioCtx )
{
	if( !c ) return WH_E_INVALIDARG;
	const wh_hparams& hp = c->m->hp;
	const int T = audioCtx > 0 ? audioCtx : hp.n_audio_ctx;
	if( T > hp.n_audio_ctx ) { setError( "audio_ctx exceeds the model's n_audio_ctx" ); return WH_E_INVALIDARG; }
	if( T == c->T ) return 0;
	WH_BIND( c->m );
	WH_HIP( hipStreamSynchronize( c->stream ) );
	// every launch reads the key count from the context (row strides of the caches included), so the override is the context's T; what was captured or
	// encoded with another T is void
	c->destroyStepGraphs();
	c->T = T;
	c->Tpad = roundUp( T, 256 );
	c->encoded = false;
	// the convolutions' zero padding sits right behind the last frame: rows 2 T + 1 of the conv input and of conv1's output may hold a longer window's data
	for( int b = 0; b < c->encChunk; b++ )
	{
		WH_HIP( hipMemsetAsync( c->convIn + b * c->convInStride + ( 2ll * T + 1 ) * hp.n_mels, 0, (size_t)hp.n_mels * 2, c->stream ) );
		WH_HIP( hipMemsetAsync( c->conv1Out + b * c->conv1Stride + ( 2ll * T + 1 ) * hp.n_audio_state, 0, (size_t)hp.n_audio_state * 2, c->stream ) );
	}
	// ... and the V operand's key padding [T, Tpad) must be finite and is expected to be zero
	WH_HIP( hipMemsetAsync( c->vT, 0, (size_t)c->encChunk * hp.n_audio_head * HEAD_DIM * roundUp( hp.n_audio_ctx, 256 ) * 2, c->stream ) );
	return 0;
}

int wh_context_set_flags( wh_context* c, uint32_t flags, int parityThreads )
{
	if( !c ) return WH_E_INVALIDARG;
	WH_CHECK( filtersAllowFlags( c, flags ) );
	c->flags = flags;
	// WH_FLAG_PARITY_EXACT with 0 threads: the decoder's P.V as ONE correctly rounded sum per output (double accumulation) instead of the reference's
	// FP16 accumulation -- the thread-count-independent value every thread count of the reference approximates
	c->parityThreads = parityThreads > 0 ? parityThreads : ( ( flags & WH_FLAG_PARITY_EXACT ) && parityThreads == 0 ? 0 : 1 );
	return 0;
}

// ---- plain device buffers for host code that must not include HIP headers (replaces Whisper/D3D/createBuffer.cpp) ----
// With WH_DEBUG_POISON set these buffers get the same treatment as the context's own: poison fill, guard regions on both
// sides, guards verified by wh_buffer_free.
namespace
{
	std::mutex g_guardedMutex;
	std::map<void*, Allocation> g_guarded;
}
int wh_buffer_alloc( int64_t bytes, void** dev )
{
	if( !dev || bytes <= 0 ) { setError( "buffer_alloc: bad argument" ); return WH_E_INVALIDARG; }
	Allocation a;
	const hipError_t e = guardedAlloc( a, bytes, wh_context::debugPoison(), nullptr, nullptr );
	if( e != hipSuccess ) { hipFail( e, "hipMalloc", __FILE__, __LINE__ ); return e == hipErrorOutOfMemory ? WH_E_OUTOFMEMORY : WH_E_HIP; }
	if( a.body != a.base )
	{
		WH_HIP( hipStreamSynchronize( nullptr ) );	   // the fills went to the null stream, the caller's work goes to streams that do not wait for it
		std::lock_guard<std::mutex> lock( g_guardedMutex );
		g_guarded.erase( a.body );
		g_guarded.emplace( a.body, a );
	}
	*dev = a.body;
	return 0;
}

int wh_buffer_free( void* dev )
{
	if( !dev ) return 0;
	Allocation a = { dev, dev, 0, nullptr };
	if( wh_context::debugGuardBytes() )
	{
		std::lock_guard<std::mutex> lock( g_guardedMutex );
		auto it = g_guarded.find( dev );
		if( it != g_guarded.end() ) { a = it->second; g_guarded.erase( it ); }
	}
	const int rc = guardedFree( a );
	return rc < 0 ? rc : 0;
}

int wh_buffer_upload( wh_context* c, void* dev, const void* host, int64_t bytes )
{
	if( !c || !dev || !host || bytes < 0 ) { setError( "buffer_upload: bad argument" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	WH_HIP( hipMemcpyAsync( dev, host, (size_t)bytes, hipMemcpyHostToDevice, c->stream ) );
	WH_HIP( hipStreamSynchronize( c->stream ) );
	return 0;
}

int wh_buffer_upload_async( wh_context* c, void* dev, const void* host, int64_t bytes )
{
	if( !c || !dev || !host || bytes < 0 ) { setError( "buffer_upload_async: bad argument" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	WH_HIP( hipMemcpyAsync( dev, host, (size_t)bytes, hipMemcpyHostToDevice, c->stream ) );
	return 0;
}

int wh_buffer_download( wh_context* c, void* host, const void* dev, int64_t bytes )
{
	if( !c || !dev || !host || bytes < 0 ) { setError( "buffer_download: bad argument" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	WH_HIP( hipMemcpyAsync( host, dev, (size_t)bytes, hipMemcpyDeviceToHost, c->stream ) );
	WH_HIP( hipStreamSynchronize( c->stream ) );
	return 0;
}

int wh_context_synchronize( wh_context* c )
{
	if( !c ) return WH_E_INVALIDARG;
	WH_BIND( c->m );
	WH_HIP( hipStreamSynchronize( c->stream ) );
	return 0;
}

int wh_context_memory( const wh_context* c, int64_t* vramBytes )
{
	if( !c || !vramBytes ) return WH_E_INVALIDARG;
	*vramBytes = c->vram;
	return 0;
}

int wh_mel_spectrogram( wh_context* c, const float* pcmDev, int64_t nSamples, float* melDev, int64_t* nLenOut )
{
	if( !c || nSamples < 0 ) { setError( "mel: bad argument" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	const int64_t nLen = nSamples / 160;
	if( nLenOut ) *nLenOut = nLen;
	if( nLen == 0 ) return 0;	// less than one hop of audio: an empty spectrogram, like the reference (whisper.cpp:2080)
	if( !pcmDev || !melDev ) { setError( "mel: null buffer" ); return WH_E_INVALIDARG; }
	const wh_model* m = c->m;
	return profiled( c, KC_MEL, 2.0 * 2.0 * 400.0 * 201.0 * nLen, 4.0 * nSamples + 4.0 * 2.0 * nLen * m->hp.n_mels,
		[ & ]() { return launchMel( pcmDev, nSamples, m->at<float>( m->L.filters ), m->at<double>( m->L.dft ), melDev, nLen, m->hp.n_mels, c->melScratch, c->stream ); } );
}

int wh_mel_spectrogram_batch( wh_context* c, const float* pcmDev, int64_t nSamples, int64_t pcmStride, int batch, float* melDev, int64_t melStride )
{
	if( !c || nSamples < 0 || batch < 0 || pcmStride < 0 || melStride < 0 ) { setError( "mel_batch: bad argument" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	const int64_t nLen = nSamples / 160;
	if( nLen == 0 || batch == 0 ) return 0;
	if( !pcmDev || !melDev ) { setError( "mel_batch: null buffer" ); return WH_E_INVALIDARG; }
	const wh_model* m = c->m;
	if( melStride < nLen * m->hp.n_mels || pcmStride < nSamples ) { setError( "mel_batch: buffers overlap" ); return WH_E_INVALIDARG; }
	for( int b0 = 0; b0 < batch; b0 += MEL_BATCH_MAX )
	{
		const int nb = batch - b0 < MEL_BATCH_MAX ? batch - b0 : MEL_BATCH_MAX;
		const float* const pcm = pcmDev + (int64_t)b0 * pcmStride;
		float* const mel = melDev + (int64_t)b0 * melStride;
		int covered = 0;
		const int rc = profiled( c, KC_MEL, 2.0 * 2.0 * 400.0 * 201.0 * nLen * nb, ( 4.0 * nSamples + 4.0 * 2.0 * nLen * m->hp.n_mels ) * nb,
			[ & ]() {
				covered = launchMelBatch( pcm, nSamples, pcmStride, nb, m->at<float>( m->L.filters ), m->at<double>( m->L.dft ), mel, melStride, nLen, m->hp.n_mels, c->melScratch + 16, c->stream );
				return covered == 1 ? 0 : covered; } );
		if( rc ) return rc;
		if( covered == 1 )
			for( int b = 0; b < nb; b++ )
			{
				const int r1 = wh_mel_spectrogram( c, pcm + (int64_t)b * pcmStride, nSamples, mel + (int64_t)b * melStride, nullptr );
				if( r1 ) return r1;
			}
	}
	return 0;
}

int wh_mel_spectrogram_window( wh_context* c, const float* pcmDev, int64_t nSamples, int64_t frame0, int64_t nFrames, int64_t nChunks,
	int reusePreviousMax, float* melDev )
{
	if( !c || nSamples < 0 || frame0 < 0 || nFrames < 0 ) { setError( "mel_window: bad argument" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	if( nFrames == 0 ) return 0;
	if( !pcmDev || !melDev ) { setError( "mel_window: null buffer" ); return WH_E_INVALIDARG; }
	const wh_model* m = c->m;
	// frame f of the stream starts at sample f * 160; frames at or beyond the reader's chunk count are zero before normalisation
	const int64_t first = frame0 * 160;
	const int64_t remaining = nSamples > first ? nSamples - first : 0;
	int64_t valid = nChunks - frame0;
	valid = valid < 0 ? 0 : ( valid > nFrames ? nFrames : valid );
	return profiled( c, KC_MEL, 2.0 * 2.0 * 400.0 * 201.0 * nFrames, 4.0 * 160.0 * nFrames + 4.0 * 2.0 * nFrames * m->hp.n_mels,
		[ & ]() { return launchMelWindow( pcmDev + ( remaining > 0 ? first : 0 ), remaining, m->at<float>( m->L.filters ), m->at<double>( m->L.dft ), melDev,
			nFrames, valid, m->hp.n_mels, reusePreviousMax, c->melScratch, c->stream ); } );
}

}	// extern "C"
