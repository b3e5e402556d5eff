// The decoder graph, host-stepped decoding (wh_decode), language detection, the sampler step, the greedy loop and its window.
#include "runtime.h"

static int attnDecP( wh_context* c, const DecAttnArgs& a, int keysHint = -1 )
{
	// ALGORITHMIC work of one launch: every K and V row the queries can see, once per (K/V block, head) -- the rows of a
	// prompt step and the hypotheses of a window share them -- with the real key count (keysHint when the position lives
	// in device memory), plus q in and the attention rows out. With a fused query also the residual rows and the query weight once.
	const int group = a.group > 0 ? a.group : 1;
	const double keys = (double)( keysHint > 0 ? keysHint : a.nKeys );
	const double d = (double)a.H * HEAD_DIM;
	double bytes = 2.0 * 2.0 * ( a.batch / group ) * a.H * keys * HEAD_DIM + 2.0 * 2.0 * a.batch * a.nTok * d;
	double flops = 4.0 * a.batch * a.H * keys * HEAD_DIM * a.nTok;
	if( a.lnX )
	{
		bytes += 4.0 * a.batch * a.nTok * d + 2.0 * d * d;
		flops += 2.0 * a.batch * a.nTok * d * d;
	}
	return profiled( c, a.causal ? KC_ATTN_DEC : KC_ATTN_DEC_CROSS, flops, bytes, [ & ]() { return launchAttentionDec( a, c->stream ); } );
}

// ------------------------------------------------------------------------------------------------------------------
// decoder
// ------------------------------------------------------------------------------------------------------------------
// The decoder graph up to the logits of the last token of every sequence. With devState the position comes from device
// memory (c->seqPos, one per sequence), which makes the launch sequence identical for every token: that is what gets captured
// into a hipGraph by wh_decode_greedy. Single-token steps of up to 16 sequences take the gemv path (weights streamed
// once, all loads of a wave in flight, LayerNorm fused into the product that consumes it); anything larger (prompt
// steps) takes the M <= 32 skinny or the tiled kernel.
int wh::decodeGraph( wh_context* c, int batch, int nTokens, int nPast, bool devState )
{
	if( c->flags & WH_FLAG_PARITY_EXACT ) { setError( "WH_FLAG_PARITY_EXACT: host-stepped decoding only (wh_decode + wh_sample_best)" ); return WH_E_INVALIDARG; }
	const wh_model* m = c->m;
	const wh_hparams& hp = m->hp;
	const Layout& L = m->L;
	hipStream_t st = c->stream;
	const int d = hp.n_text_state, H = hp.n_text_head;
	const int M = batch * nTokens;
	const float kqScale = (float)pow( (double)( (float)d / (float)H ), -0.25 );
	const int parity = ( c->flags & WH_FLAG_PARITY_PV ) ? c->parityThreads : 0;
	const int* const nPastDev = devState ? c->seqPos : nullptr;
	// the weight-streaming kernels (gemvFused up to 128 rows, gemmDecRows up to 512) are sized and tuned for single-token steps of a lock-step batch; a PROMPT
	// step of 129 .. 512 rows (one stream with a carried-over prompt of ~224 tokens, small batches with a prompt) keeps the M-tiled MFMA kernel it always had
	// (raising GEMV_MAX_ROWS to 512 had silently re-routed those, summation order included)
	const bool gemv = M <= ( nTokens == 1 ? GEMV_MAX_ROWS : GEMV_FUSED_MAX_ROWS ) && ( d % 128 ) == 0;
	const bool fuseLn = gemv && d <= 1280 && M <= 32 && ( M <= 16 || ( g_tuning & TUNE_GEMV_LN_BLOCK ) || !( g_tuning & TUNE_LN_SEPARATE_BIGM ) );
	// decode steps: LayerNorm + this head's Q/K/V rows + cache append + self-attention in one launch
	// (from 9 sequences up: with fewer, one workgroup per (head, sequence) leaves the 6 d^2 bytes of QKV weights to H CUs at
	// ~25 GB/s each -- 15.7 us per layer at one sequence -- and the separate gemv + attention launches are faster: 74.3 vs 86.6 ms
	// per window at batch 1, 100.4 vs 101.9 at 7)
	const bool fuseSelf = nTokens == 1 && d <= 1280 && hp.n_text_ctx <= 512 && parity == 0 && batch > 8 && batch <= g_opt.selfFuseMaxRows && ( g_tuning & TUNE_FUSE_SELF_BLOCK );
	// decode steps: the cross-attention kernel normalises the residual row and projects its own head's query
	const bool fuseCrossQ = nTokens == 1 && d <= 1280 && parity <= 8 && ( g_tuning & TUNE_FUSE_CROSS_Q );

	auto product = [ & ]( GemmArgs& g, const float* lnW, const float* lnB ) -> int
	{
		g.nPastDev = nPastDev;
		if( !gemv ) return gemmP( c, g, true, true );
		if( g.N <= d ) g.splitScratch = c->splitK;
		if( lnW && fuseLn )
		{
			g.lnX = c->dx; g.lnW = lnW; g.lnB = lnB;
		}
		const double flops = 2.0 * g.M * g.N * g.K;
		const double bytes = 2.0 * g.N * g.K + 2.0 * g.M * g.K + ( g.out32 ? 4.0 : 2.0 ) * g.M * g.N;
		return profiled( c, KC_GEMV, flops, bytes, [ & ]() { return launchGemv( g, st ); } );
	};

	WH_CHECK( profiled( c, KC_EMBED, 1.0 * M * d, 10.0 * M * d,
		[ & ]() { return launchEmbed( c->tokensDev, m->at<f16>( L.te ), m->at<float>( L.decPe ), c->dx, M, nTokens, nPast, nPastDev, d, hp.n_vocab, hp.n_text_ctx, st ); } ) );

	// ---- single-token steps of up to 4 sequences (one stream through iContext::runFull): decode1.hip. Eight launches per layer,
	// each of ~256 workgroups, each pulling the weights of the next one into the L2 of the XCD that will read them.
	const bool small = nTokens == 1 && batch <= SMALL_MAX_ROWS && c->hyp == 1 && parity == 0 && d <= 1280 && ( d % 64 ) == 0 && c->T <= 1536 &&
		!( c->flags & WH_FLAG_DEBUG_CAPTURE ) && ( g_tuning & TUNE_DECODE_SMALL );
	if( small )
	{
#ifdef WH_PROBES
		const bool pfOn = ( g_tuning & TUNE_DECODE_PREFETCH ) != 0;	   // measured slower: a probe build's switch only
#else
		const bool pfOn = false;
#endif
		// what a gemvSmall launch of N rows x K columns streams per workgroup (must mirror launchGemvSmall's row split)
		auto gemvChunk = [ & ]( int N, int K ) -> int
		{
			const int nch = ( K + 511 ) >> 9;
			int rw = ( N + 1023 ) / 1024;
			if( rw < 1 ) rw = 1;
			const int mr = batch <= 2 ? batch : 4;
			while( rw > 1 && ( rw * nch > 16 || rw * 4 * mr > 64 ) ) rw--;
			return rw * 4 * K * 2;
		};
		auto hint = [ & ]( const void* p, int64_t bytes, int chunk ) -> PrefetchHint
		{
			PrefetchHint h = { nullptr, 0, 0 };
			if( pfOn ) { h.ptr = p; h.bytes = bytes; h.chunkBytes = chunk; }
			return h;
		};
		auto smallGemv = [ & ]( SmallGemvArgs& a ) -> int
		{
			a.g.nPastDev = nPastDev;
			const GemmArgs& g = a.g;
			const double flops = 2.0 * g.M * g.N * g.K;
			const double bytes = 2.0 * g.N * g.K + 2.0 * g.M * g.K + ( g.out32 ? 4.0 : 2.0 ) * g.M * g.N;
			return profiled( c, KC_GEMV, flops, bytes, [ & ]() { return launchGemvSmall( a, st ); } );
		};
		const int64_t headKv = (int64_t)c->T * HEAD_DIM * 2;	   // bytes of one (sequence, head) of a cross-attention cache
		for( int il = 0; il < hp.n_text_layer; il++ )
		{
			const DecLayer& e = L.dec[ il ];
			const int64_t selfLayer = (int64_t)il * c->maxSeq * hp.n_text_ctx * d;
			const int64_t crossLayer = (int64_t)il * c->maxBatch * c->T * d;
			// 1. LayerNorm + Q/K/V (cache append)                          next but one: the self-attention output projection
			{
				SmallGemvArgs a = {};
				a.g = plainGemm( nullptr, m->at<f16>( e.wqkv ), M, 3 * d, d );
				a.g.epi = EPI_QKV_DEC; a.g.bias = m->at<float>( e.bqkv ); a.g.scale = kqScale;
				a.g.q = c->dq; a.g.k = c->selfK + selfLayer; a.g.v = c->selfV + selfLayer;
				a.g.H = H; a.g.nTok = 1; a.g.nPast = nPast; a.g.textCtx = hp.n_text_ctx;
				a.pro = 1; a.g.lnX = c->dx; a.g.lnW = m->at<float>( e.ln1w ); a.g.lnB = m->at<float>( e.ln1b );
				a.pf[ 0 ] = hint( m->at<f16>( e.wo ), (int64_t)d * d * 2, gemvChunk( d, d ) );
				WH_CHECK( smallGemv( a ) );
			}
			// 2. self-attention (a head per workgroup: at most n_text_ctx keys)
			{
				DecAttnArgs a = {};
				a.q = c->dq; a.kc = c->selfK + selfLayer; a.vc = c->selfV + selfLayer; a.out = c->dattn;
				a.batch = batch; a.H = H; a.nTok = 1; a.nKeys = nPast + 1; a.keyStride = hp.n_text_ctx;
				a.causal = 1; a.nPast = nPast; a.parityThreads = 0; a.nPastDev = nPastDev;
				if( devState ) a.nKeys = hp.n_text_ctx;
				WH_CHECK( attnDecP( c, a, devState ? c->profKeysHint : -1 ) );
				if( il == 0 && !devState && !c->alignHook )
				{
					WH_CHECK( capture( c, c->capDecKqvSelf, c->dattn, (int64_t)M * d, (int64_t)c->maxRows * d ) );	 // "dec-KQV" (self)
					c->capDecRows = M;
				}
			}
			// 3. output projection + residual                              next: the query rows and the keys of the cross-attention
			{
				SmallGemvArgs a = {};
				a.g = plainGemm( c->dattn, m->at<f16>( e.wo ), M, d, d );
				a.g.epi = EPI_F32; a.g.bias = m->at<float>( e.bo ); a.g.res = c->dx; a.g.out32 = c->dx;
				a.pf[ 0 ] = hint( m->at<f16>( e.wcq ), (int64_t)d * d * 2, HEAD_DIM * d * 2 );
				a.pf[ 1 ] = hint( c->crossK + crossLayer, (int64_t)batch * H * headKv, (int)headKv );
				WH_CHECK( smallGemv( a ) );
			}
			// 4. / 5. cross-attention over 8 key ranges per head            next: the values, then the output projection
			CrossSplitArgs x = {};
			x.lnX = c->dx; x.lnW = m->at<float>( e.lncw ); x.lnB = m->at<float>( e.lncb );
			x.qW = m->at<f16>( e.wcq ); x.qB = m->at<float>( e.bcq ); x.qScale = kqScale;
			x.kc = c->crossK + crossLayer; x.vc = c->crossV + crossLayer;
			x.scores = c->crossScores; x.splitMax = c->crossSplitMax; x.part = c->crossPart;
			x.batch = batch; x.H = H; x.nKeys = c->T; x.keyStride = c->T;
			{
				const double bytes = 2.0 * d * d + 2.0 * M * c->T * d + 4.0 * M * d;
				x.pf[ 0 ] = hint( c->crossV + crossLayer, (int64_t)batch * H * headKv, (int)headKv );
				WH_CHECK( profiled( c, KC_ATTN_DEC_CROSS, 2.0 * M * d * d + 2.0 * M * c->T * d, bytes, [ & ]() { return launchCrossScores( x, st ); } ) );
				x.pf[ 0 ] = hint( m->at<f16>( e.wco ), (int64_t)d * d * 2, gemvChunk( d, d ) );
				WH_CHECK( profiled( c, KC_ATTN_DEC_CROSS, 2.0 * M * c->T * d, 2.0 * M * c->T * d + 4.0 * M * H * c->T, [ & ]() { return launchCrossSoftmaxPV( x, st ); } ) );
			}
			// 6. splits combined + output projection + residual              next: the MLP up-projection
			{
				SmallGemvArgs a = {};
				a.g = plainGemm( nullptr, m->at<f16>( e.wco ), M, d, d );
				a.g.epi = EPI_F32; a.g.bias = m->at<float>( e.bco ); a.g.res = c->dx; a.g.out32 = c->dx;
				a.pro = 3; a.part = c->crossPart;
				a.pf[ 0 ] = hint( m->at<f16>( e.w1 ), (int64_t)4 * d * d * 2, gemvChunk( 4 * d, d ) );
				WH_CHECK( smallGemv( a ) );
			}
			// 7. LayerNorm + MLP up + GELU                                    next: the MLP down-projection
			{
				SmallGemvArgs a = {};
				a.g = plainGemm( nullptr, m->at<f16>( e.w1 ), M, 4 * d, d );
				a.g.epi = EPI_F16_GELU; a.g.bias = m->at<float>( e.b1 ); a.g.out16 = c->dh;
				a.pro = 1; a.g.lnX = c->dx; a.g.lnW = m->at<float>( e.ln2w ); a.g.lnB = m->at<float>( e.ln2b );
				a.pf[ 0 ] = hint( m->at<f16>( e.w2 ), (int64_t)4 * d * d * 2, gemvChunk( d, 4 * d ) );
				WH_CHECK( smallGemv( a ) );
			}
			// 8. MLP down + residual                                          next: the following layer's Q/K/V rows
			{
				SmallGemvArgs a = {};
				a.g = plainGemm( c->dh, m->at<f16>( e.w2 ), M, d, 4 * d );
				a.g.epi = EPI_F32; a.g.bias = m->at<float>( e.b2 ); a.g.res = c->dx; a.g.out32 = c->dx;
				if( il + 1 < hp.n_text_layer )
					a.pf[ 0 ] = hint( m->at<f16>( L.dec[ il + 1 ].wqkv ), (int64_t)3 * d * d * 2, gemvChunk( 3 * d, d ) );
				WH_CHECK( smallGemv( a ) );
			}
		}
		// final norm fused into the vocabulary projection's prologue (1621 workgroups normalise one row each: 4 KB from L2)
		{
			SmallGemvArgs a = {};
			a.g = plainGemm( nullptr, m->at<f16>( L.te ), batch, hp.n_vocab, d );
			a.g.epi = EPI_F32; a.g.out32 = c->logits; a.g.ldc = hp.n_vocab;
			a.pro = 1; a.g.lnX = c->dx; a.g.lnW = m->at<float>( L.decLnW ); a.g.lnB = m->at<float>( L.decLnB );
			WH_CHECK( smallGemv( a ) );
		}
		return filterLogits( c, batch );
	}

	for( int il = 0; il < hp.n_text_layer; il++ )
	{
		const DecLayer& e = L.dec[ il ];
		const int64_t selfLayer = (int64_t)il * c->maxSeq * hp.n_text_ctx * d;
		const int64_t crossLayer = (int64_t)il * c->maxBatch * c->T * d;
		// self-attention
		if( fuseSelf )
		{
			DecSelfArgs a = {};
			a.x = c->dx; a.lnW = m->at<float>( e.ln1w ); a.lnB = m->at<float>( e.ln1b );
			a.wqkv = m->at<f16>( e.wqkv ); a.bqkv = m->at<float>( e.bqkv ); a.scale = kqScale;
			a.kc = c->selfK + selfLayer; a.vc = c->selfV + selfLayer; a.out = c->dattn;
			a.batch = batch; a.H = H; a.keyStride = hp.n_text_ctx; a.nPast = nPast; a.nPastDev = nPastDev;
			const double keys = devState ? c->profKeysHint : nPast + 1;
			// algorithmic: the fused [3d][d] weight once, the residual rows, the cached K and V rows, the appended rows, the output
			const double bytes = 2.0 * 3.0 * d * d + 4.0 * M * d + 2.0 * 2.0 * M * ( keys - 1 ) * d + 2.0 * 2.0 * M * d + 2.0 * M * d;
			const double flops = 2.0 * M * 3.0 * d * d + 4.0 * M * keys * d;
			WH_CHECK( profiled( c, KC_SELF_BLOCK, flops, bytes, [ & ]() { return launchSelfBlockDec( a, st ); } ) );
			if( il == 0 && !devState && !c->alignHook && !c->scoreHook )
			{
				WH_CHECK( capture( c, c->capDecKqvSelf, c->dattn, (int64_t)M * d, (int64_t)c->maxRows * d ) );	 // "dec-KQV" (self)
				c->capDecRows = M;
			}
		}
		else
		{
		if( !fuseLn ) WH_CHECK( lnP( c, c->dx, m->at<float>( e.ln1w ), m->at<float>( e.ln1b ), c->dxn, M, d, true ) );
		{
			GemmArgs g = plainGemm( c->dxn, m->at<f16>( e.wqkv ), M, 3 * d, d );
			g.epi = EPI_QKV_DEC;
			g.bias = m->at<float>( e.bqkv );
			g.scale = kqScale;
			g.q = c->dq; g.k = c->selfK + selfLayer; g.v = c->selfV + selfLayer;
			g.H = H; g.nTok = nTokens; g.nPast = nPast; g.textCtx = hp.n_text_ctx;
			WH_CHECK( product( g, m->at<float>( e.ln1w ), m->at<float>( e.ln1b ) ) );
		}
		{
			DecAttnArgs a = {};
			a.q = c->dq; a.kc = c->selfK + selfLayer; a.vc = c->selfV + selfLayer; a.out = c->dattn;
			a.batch = batch; a.H = H; a.nTok = nTokens; a.nKeys = nPast + nTokens; a.keyStride = hp.n_text_ctx;
			a.causal = 1; a.nPast = nPast; a.parityThreads = parity; a.nPastDev = nPastDev;
			if( devState ) a.nKeys = hp.n_text_ctx;	  // upper bound for the argument check; the kernel reads the real value
			WH_CHECK( attnDecP( c, a, devState ? c->profKeysHint : -1 ) );
			if( il == 0 && !devState && !c->alignHook && !c->scoreHook )
			{
				WH_CHECK( capture( c, c->capDecKqvSelf, c->dattn, (int64_t)M * d, (int64_t)c->maxRows * d ) );	 // "dec-KQV" (self)
				c->capDecRows = M;
			}
		}
		}
		{
			GemmArgs g = plainGemm( c->dattn, m->at<f16>( e.wo ), M, d, d );
			g.epi = EPI_F32; g.bias = m->at<float>( e.bo ); g.res = c->dx; g.out32 = c->dx;
			WH_CHECK( product( g, nullptr, nullptr ) );
		}
		// cross-attention
		if( !fuseCrossQ )
		{
			if( !fuseLn ) WH_CHECK( lnP( c, c->dx, m->at<float>( e.lncw ), m->at<float>( e.lncb ), c->dxn, M, d, true ) );
			GemmArgs g = plainGemm( c->dxn, m->at<f16>( e.wcq ), M, d, d );
			g.epi = EPI_Q_DEC; g.bias = m->at<float>( e.bcq ); g.scale = kqScale; g.q = c->dq;
			WH_CHECK( product( g, m->at<float>( e.lncw ), m->at<float>( e.lncb ) ) );
		}
		if( const AlignHook* const hook = c->alignHook; hook && il >= hook->layer0 )
		{
			// wh_align_tokens: this layer's query rows, and the end of the pass behind the last selected layer
			if( fuseCrossQ ) { setError( "align_tokens: the query rows of a single-token step are never formed" ); return WH_E_INVALIDARG; }
			WH_HIP( hipMemcpyAsync( hook->q + (int64_t)( il - hook->layer0 ) * hook->layerStride, c->dq, sizeof( f16 ) * (size_t)M * d, hipMemcpyDeviceToDevice, st ) );
			if( il >= hook->layer1 ) return 0;
		}
		{
			DecAttnArgs a = {};
			a.q = c->dq; a.kc = c->crossK + crossLayer; a.vc = c->crossV + crossLayer; a.out = c->dattn;
			a.batch = batch; a.H = H; a.nTok = nTokens; a.nKeys = c->T; a.keyStride = c->T;
			a.causal = 0; a.nPast = 0; a.parityThreads = parity; a.nPastDev = nullptr;
			a.group = c->hyp;
			// the rows of a multi-token (prompt) step see the same keys -- there is no causal mask across the encoder output --
			// so they are to the kernel what the hypotheses of a window are: one pass over the window's K/V for all of them
			// (as separate query tokens every token's workgroup re-read it: 2.4 GB instead of 0.69 GB per launch at 112 windows)
			{
				const int rowsPerWindow = c->hyp * nTokens;
				const bool groupable = rowsPerWindow <= 5 || rowsPerWindow == 8;
				if( nTokens > 1 && parity == 0 && groupable )
				{
					a.batch = batch * nTokens; a.nTok = 1; a.group = rowsPerWindow;
				}
			}
			if( fuseCrossQ )
			{
				a.lnX = c->dx; a.lnW = m->at<float>( e.lncw ); a.lnB = m->at<float>( e.lncb );
				a.qW = m->at<f16>( e.wcq ); a.qB = m->at<float>( e.bcq ); a.qScale = kqScale;
			}
			WH_CHECK( attnDecP( c, a ) );
			if( il == 0 && !devState && !c->alignHook && !c->scoreHook ) WH_CHECK( capture( c, c->capDecKqvCross, c->dattn, (int64_t)M * d, (int64_t)c->maxRows * d ) );	  // "dec-KQV" (cross)
		}
		{
			GemmArgs g = plainGemm( c->dattn, m->at<f16>( e.wco ), M, d, d );
			g.epi = EPI_F32; g.bias = m->at<float>( e.bco ); g.res = c->dx; g.out32 = c->dx;
			WH_CHECK( product( g, nullptr, nullptr ) );
		}
		// MLP
		if( !fuseLn ) WH_CHECK( lnP( c, c->dx, m->at<float>( e.ln2w ), m->at<float>( e.ln2b ), c->dxn, M, d, true ) );
		{
			GemmArgs g = plainGemm( c->dxn, m->at<f16>( e.w1 ), M, 4 * d, d );
			g.epi = EPI_F16_GELU; g.bias = m->at<float>( e.b1 ); g.out16 = c->dh;
			WH_CHECK( product( g, m->at<float>( e.ln2w ), m->at<float>( e.ln2b ) ) );
		}
		{
			GemmArgs g = plainGemm( c->dh, m->at<f16>( e.w2 ), M, d, 4 * d );
			g.epi = EPI_F32; g.bias = m->at<float>( e.b2 ); g.res = c->dx; g.out32 = c->dx;
			WH_CHECK( product( g, nullptr, nullptr ) );
		}
	}
	// final norm + logits for the LAST token of every sequence only (the reference computes all rows, whisper.cpp:1840,
	// and then consumes just the last one, ContextImpl.cpp:159-169). The norm stays a separate launch here: fusing it
	// into the 3242 workgroups of the vocabulary product would re-read the rows 3242 times.
	WH_CHECK( lnP( c, c->dx, m->at<float>( L.decLnW ), m->at<float>( L.decLnB ), c->dxn, M, d, true ) );
	// wh_score_tokens: all M normalised rows are the result; the caller gathers the ones it scores and runs the vocabulary product on them
	if( c->scoreHook ) return 0;
	// prompts of different lengths (rows right-padded to nTokens): the row of every sequence's own last token moves to where the
	// product below reads, row nTokens - 1 of the sequence
	if( c->raggedLastPos && nTokens > 1 ) WH_CHECK( launchGatherLastRows( c->dxn, c->raggedLastPos, batch, nTokens, d, st ) );
	{
		GemmArgs g = plainGemm( c->dxn + (int64_t)( nTokens - 1 ) * d, m->at<f16>( L.te ), batch, hp.n_vocab, d );
		g.lda = nTokens * d;
		g.epi = EPI_F32; g.out32 = c->logits; g.ldc = hp.n_vocab;
		// more than 128 sequences: the vocabulary matrix (106 / 133 MB) against that many rows is a GEMM of ~50 GFLOP whose weight tiles should be
		// fetched once: the M-tiled kernel (128 x 128 tiles, 400 column tiles x ceil(batch / 128) row tiles)
		// (option vocab_decrows: gemmDecRows instead, for A/B runs)
		if( gemv && batch > GEMV_FUSED_MAX_ROWS && !g_opt.vocabDecRows )
		{
			g.nPastDev = nPastDev;
			WH_CHECK( gemmP( c, g, true, true ) );
		}
		else
			WH_CHECK( product( g, nullptr, nullptr ) );
	}
	return filterLogits( c, batch );
}

// Token ids index the embedding table: anything outside [0, n_vocab) is rejected at the boundary (the reference's addRows
// shader reads whatever the id selects, MlContext.cpp:588-618; here a bad id is the caller's error, not a device fault).
int wh::checkTokens( const wh_hparams& hp, const int32_t* tokens, int64_t count, const char* who )
{
	for( int64_t i = 0; i < count; i++ )
		if( tokens[ i ] < 0 || tokens[ i ] >= hp.n_vocab )
		{
			char buf[ 160 ];
			snprintf( buf, sizeof( buf ), "%s: token id %d at index %lld is outside [0, %d)", who, (int)tokens[ i ], (long long)i, hp.n_vocab );
			setError( buf );
			return WH_E_INVALIDARG;
		}
	return 0;
}

extern "C" {

int wh_decode( wh_context* c, const int32_t* tokens, int batch, int nTokens, int nPast, float* logitsHost, float* probsHost )
{
	if( !c || !tokens || batch <= 0 || batch > c->maxSeq || ( batch % c->hyp ) != 0 || nTokens <= 0 || nPast < 0 ) { setError( "decode: bad argument" ); return WH_E_INVALIDARG; }
	if( !c->encoded ) { setError( "decode: wh_encode has not run" ); return WH_E_NOT_READY; }
	WH_BIND( c->m );
	const wh_hparams& hp = c->m->hp;
	if( nPast + nTokens > hp.n_text_ctx ) { setError( "decode: n_past + n_tokens exceeds n_text_ctx" ); return WH_E_BOUNDS; }
	hipStream_t st = c->stream;
	const int M = batch * nTokens;
	WH_CHECK( checkTokens( hp, tokens, M, "decode" ) );
	WH_HIP( hipMemcpyAsync( c->tokensDev, tokens, sizeof( int32_t ) * M, hipMemcpyHostToDevice, st ) );
	if( c->flags & WH_FLAG_PARITY_EXACT )
		WH_CHECK( decodeExact( c, batch, nTokens, nPast ) );
	else
	{
	WH_CHECK( decodeGraph( c, batch, nTokens, nPast, false ) );
	WH_CHECK( profiled( c, KC_SOFTMAX, 10.0 * batch * hp.n_vocab, 12.0 * batch * hp.n_vocab,
		[ & ]() { return launchVocabSoftMax( c->logits, c->probs, batch, hp.n_vocab, st ); } ) );
	}
	c->lastBatch = batch;
	if( logitsHost ) WH_HIP( hipMemcpyAsync( logitsHost, c->logits, sizeof( float ) * batch * hp.n_vocab, hipMemcpyDeviceToHost, st ) );
	if( probsHost ) WH_HIP( hipMemcpyAsync( probsHost, c->probs, sizeof( float ) * batch * hp.n_vocab, hipMemcpyDeviceToHost, st ) );
	if( logitsHost || probsHost ) WH_HIP( hipStreamSynchronize( st ) );
	return 0;
}

// Language tokens of a vocabulary: sot + 1 .. sot + n_lang, n_lang = n_vocab - 51766 (99 at 51865, 100 at the large-v3 shape); none below 51865 (.en models)
static int langCount( const wh_hparams& hp ) { return hp.n_vocab >= 51865 ? hp.n_vocab - 51766 : 0; }

int wh_model_lang_count( const wh_model* m )
{
	if( !m ) { setError( "model_lang_count: null model" ); return WH_E_INVALIDARG; }
	return langCount( m->hp );
}

// whisper_lang_auto_detect (Whisper/source/whisper.cpp:2428-2495) for the windows of the last wh_encode: [sot] at position 0, the probabilities of the
// language tokens. A one-token step of the context's ordinary route; on a hypothesis-group context every sequence of a group runs the step (the groups share
// their cross-attention pass) and the group's first row is read. Nothing of the context's decoding state depends on a host-stepped decode: position 0 of the
// self-attention caches is rewritten by the prompt of whatever decodes next.
int wh_lang_detect( wh_context* c, int batch, float* langP, int32_t* best )
{
	if( !c || !best || batch <= 0 || batch > c->maxBatch ) { setError( "lang_detect: bad argument" ); return WH_E_INVALIDARG; }
	if( !c->encoded ) { setError( "lang_detect: wh_encode has not run" ); return WH_E_NOT_READY; }
	if( batch > c->lastEncBatch ) { setError( "lang_detect: more windows than the last wh_encode filled" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	const wh_hparams& hp = c->m->hp;
	const int nLang = langCount( hp );
	if( nLang <= 0 ) { setError( "lang_detect: the model is not multilingual" ); return WH_E_INVALIDARG; }
	hipStream_t st = c->stream;
	const int sot = specialIds( hp ).sot;
	const int seqs = batch * c->hyp;
	if( !c->langP )
	{
		WH_CHECK( c->alloc( c->langP, (int64_t)c->maxBatch * nLang, wh_context::DONT_CARE, "langP" ) );
		WH_CHECK( c->alloc( c->langBest, (int64_t)c->maxBatch, wh_context::DONT_CARE, "langBest" ) );
	}
	int32_t* const stTok = c->pinTokens();
	if( c->pinTokenCap() < seqs ) { setError( "lang_detect: staging too small" ); return WH_E_BOUNDS; }
	WH_HIP( hipStreamSynchronize( st ) );	  // the staging may still be read by an earlier enqueue
	for( int i = 0; i < seqs; i++ ) stTok[ i ] = sot;
	WH_HIP( hipMemcpyAsync( c->tokensDev, stTok, sizeof( int32_t ) * seqs, hipMemcpyHostToDevice, st ) );
	const long long rowStride = (long long)c->hyp * hp.n_vocab;
	if( c->flags & WH_FLAG_PARITY_EXACT )
	{
		WH_CHECK( decodeExact( c, seqs, 1, 0 ) );
		WH_CHECK( launchLangGather( c->probs, rowStride, batch, hp.n_vocab, sot, nLang, c->langP, c->langBest, st ) );
	}
	else
	{
		// detection is the model's own distribution at [sot]: the pass runs unfiltered whatever set the context holds (set around the call like AlignHook)
		bypassFilterLogits( c, true );
		const int rcGraph = decodeGraph( c, seqs, 1, 0, false );
		bypassFilterLogits( c, false );
		WH_CHECK( rcGraph );
		WH_CHECK( profiled( c, KC_SOFTMAX, 10.0 * batch * hp.n_vocab, 4.0 * batch * hp.n_vocab,
			[ & ]() { return launchLangProbs( c->logits, rowStride, batch, hp.n_vocab, sot, nLang, c->langP, c->langBest, st ); } ) );
	}
	if( langP ) WH_HIP( hipMemcpyAsync( langP, c->langP, sizeof( float ) * batch * nLang, hipMemcpyDeviceToHost, st ) );
	WH_HIP( hipMemcpyAsync( best, c->langBest, sizeof( int32_t ) * batch, hipMemcpyDeviceToHost, st ) );
	WH_HIP( hipStreamSynchronize( st ) );
	c->lastBatch = c->lastEncBatch * c->hyp;	  // as wh_encode left it
	return 0;
}

}	// extern "C"

// The sampler state and the positions of `batch` sequences -> device, through the pinned staging (asynchronous; the staging is
// reused by the next call, which callers order behind a synchronisation of their own). positions == nullptr: `uniform` for all.
int wh::uploadDecodeState( wh_context* c, int batch, const DecodeState& s, const int32_t* positions, int uniform )
{
	DecodeState* const stState = (DecodeState*)( c->pinned + wh_context::PIN_STATE );
	int32_t* const stPos = c->pinned + wh_context::PIN_POS;
	static_assert( sizeof( DecodeState ) <= sizeof( int32_t ) * ( wh_context::PIN_POS - wh_context::PIN_STATE ), "staging layout" );
	*stState = s;
	for( int i = 0; i < batch; i++ ) stPos[ i ] = positions ? positions[ i ] : uniform;
	WH_HIP( hipMemcpyAsync( c->state, stState, sizeof( DecodeState ), hipMemcpyHostToDevice, c->stream ) );
	WH_HIP( hipMemcpyAsync( c->seqPos, stPos, sizeof( int32_t ) * batch, hipMemcpyHostToDevice, c->stream ) );
	return 0;
}

// Does the spread sampler serve `batch` rows in the context's present mode? It leaves unnormalised e and its slice sums where the others leave probabilities,
// so whoever reads c->probs behind a sample asks here
static bool spreadSampler( const wh_context* c, int batch )
{
	return !c->sampleRowsOn && !( c->temperature > 0.0f ) && batch <= SMALL_MAX_ROWS && ( g_tuning & TUNE_SAMPLE_SPREAD );
}

// logits -> table softmax -> sampleBest -> token data + next token: one workgroup per row, or -- for the few rows of one stream -- every row cut
// into 64 slices over the chip (three small launches, ~12 us instead of 41 on one CU)
static int sampleStep( wh_context* c, int batch, hipStream_t st )
{
	const wh_hparams& hp = c->m->hp;
	const SpecialIds sp = specialIds( hp );
	const int sot = sp.sot, solm = sp.solm, tnot = sp.tnot, beg = sp.beg;
	if( c->sampleRowsOn )
	{
		// wh_context_set_sampling_rows: the same two one-workgroup kernels with a record per row -- a greedy row's factor is 1 and its draw ends behind sampleBest's pick
		WH_CHECK( profiled( c, KC_SOFTMAX, 11.0 * batch * hp.n_vocab, 8.0 * batch * hp.n_vocab,
			[ & ]() { return launchVocabSoftMaxRows( c->logits, c->sampleRows, c->probs, batch, hp.n_vocab, st ); } ) );
		return profiled( c, KC_SAMPLE, 4.0 * batch * hp.n_vocab, 8.0 * batch * hp.n_vocab,
			[ & ]() { return launchSampleRows( c->probs, batch, hp.n_vocab, beg, sot, solm, tnot, 0, 0, c->state, c->sampleRows, c->seqPos, c->greedyOut, c->tokensDev, c->mailDev, st ); } );
	}
	if( c->temperature > 0.0f )
	{
		// wh_context_set_sampling: the table softmax of logits / T, then one draw per row under sampleBest's masks (sample.hip), which also does the loop's bookkeeping
		WH_CHECK( profiled( c, KC_SOFTMAX, 11.0 * batch * hp.n_vocab, 8.0 * batch * hp.n_vocab,
			[ & ]() { return launchVocabSoftMaxScaled( c->logits, 1.0f, &c->sampleParams->invT, c->probs, batch, hp.n_vocab, st ); } ) );
		return profiled( c, KC_SAMPLE, 4.0 * batch * hp.n_vocab, 8.0 * batch * hp.n_vocab,
			[ & ]() { return launchSampleDrawStep( c->probs, batch, hp.n_vocab, beg, sot, solm, tnot, c->state, c->sampleParams, c->seqPos, c->greedyOut, c->tokensDev, c->mailDev, st ); } );
	}
	if( spreadSampler( c, batch ) )
	{
		if( !c->sampleScratch ) WH_CHECK( c->alloc( c->sampleScratch, (int64_t)sampleSpreadScratchBytes( SMALL_MAX_ROWS ), wh_context::DONT_CARE, "sampleScratch" ) );
		return profiled( c, KC_SAMPLE, 12.0 * batch * hp.n_vocab, 8.0 * batch * hp.n_vocab,
			[ & ]() { return launchSoftMaxSampleSpread( c->logits, c->probs, batch, hp.n_vocab, beg, sot, solm, tnot, c->state, c->greedyOut, c->tokensDev, c->mailDev, c->sampleScratch, st ); } );
	}
	return profiled( c, KC_SAMPLE, 12.0 * batch * hp.n_vocab, 8.0 * batch * hp.n_vocab,
		[ & ]() { return launchSoftMaxSample( c->logits, c->probs, batch, hp.n_vocab, beg, sot, solm, tnot, c->state, c->greedyOut, c->tokensDev, c->mailDev, st ); } );
}

// One greedy token on the device: decoder graph -> softmax + sampleBest -> advance the device-resident state.
static int greedyStep( wh_context* c, int batch )
{
	WH_CHECK( decodeGraph( c, batch, 1, 0, true ) );
	WH_CHECK( filterLoopRows( c, batch, FILTER_STEP ) );
	WH_CHECK( sampleStep( c, batch, c->stream ) );
	return launchAdvanceState( c->state, c->seqPos, batch, c->stream );
}
// Everything in device memory that a greedyStep mutates and a window in progress still needs (obtainStepGraph's WARM_PRESERVE; the stream is idle): the sampler
// state, the positions, the fed tokens, and what the filters keep per row, which is their owner's to list (filters.hip).
// (The cache row and the sample the warm-up writes are rewritten by the first real step.)
int wh::saveLoopState( wh_context* c, int batch, LoopState& s )
{
	s.pos.resize( (size_t)batch );
	s.tok.resize( (size_t)batch );
	WH_HIP( hipMemcpy( &s.state, c->state, sizeof( DecodeState ), hipMemcpyDeviceToHost ) );
	WH_HIP( hipMemcpy( s.pos.data(), c->seqPos, sizeof( int32_t ) * batch, hipMemcpyDeviceToHost ) );
	WH_HIP( hipMemcpy( s.tok.data(), c->tokensDev, sizeof( int32_t ) * batch, hipMemcpyDeviceToHost ) );
	return saveFilterState( c, batch, s.filters );
}
int wh::restoreLoopState( wh_context* c, int batch, const LoopState& s )
{
	WH_HIP( hipMemcpy( c->state, &s.state, sizeof( DecodeState ), hipMemcpyHostToDevice ) );
	WH_HIP( hipMemcpy( c->seqPos, s.pos.data(), sizeof( int32_t ) * batch, hipMemcpyHostToDevice ) );
	WH_HIP( hipMemcpy( c->tokensDev, s.tok.data(), sizeof( int32_t ) * batch, hipMemcpyHostToDevice ) );
	return restoreFilterState( c, batch, s.filters );
}

extern "C" {

int wh_decode_greedy( wh_context* c, int batch, const int32_t* firstTokens, int nPast, int nSteps, int forceFirstTimestamp, int firstIsInitial,
	wh_token_data* out )
{
	if( !c || !firstTokens || !out || batch <= 0 || batch > c->maxSeq || ( batch % c->hyp ) != 0 || nSteps <= 0 || nPast < 0 ) { setError( "decode_greedy: bad argument" ); return WH_E_INVALIDARG; }
	if( !c->encoded ) { setError( "decode_greedy: wh_encode has not run" ); return WH_E_NOT_READY; }
	WH_BIND( c->m );
	const wh_hparams& hp = c->m->hp;
	if( nPast + nSteps > hp.n_text_ctx ) { setError( "decode_greedy: n_past + n_steps exceeds n_text_ctx" ); return WH_E_BOUNDS; }
	WH_CHECK( checkTokens( hp, firstTokens, batch, "decode_greedy" ) );
	hipStream_t st = c->stream;
	const DecodeState init = { 0, forceFirstTimestamp ? 1 : 0, firstIsInitial ? 1 : 0, 0 };
	WH_HIP( hipStreamSynchronize( st ) );	 // the staging may still be read by an earlier enqueue
	WH_CHECK( uploadDecodeState( c, batch, init, nullptr, nPast ) );
	WH_HIP( hipMemcpyAsync( c->tokensDev, firstTokens, sizeof( int32_t ) * batch, hipMemcpyHostToDevice, st ) );
	WH_HIP( hipStreamSynchronize( st ) );

	const StepFn step = [ c, batch ]() { return greedyStep( c, batch ); };
	hipGraphExec_t exec = nullptr;
	// nPast may be above 0 over the cache rows of an earlier wh_decode, and the state is uploaded: the warm-up must preserve both
	if( stepsReplayable( c ) ) WH_CHECK( obtainStepGraph( c, batch, stepKey( c, 0 ), WARM_PRESERVE, nullptr, step, exec ) );
	// the first token is the caller's, not a sample: the filters' histories are armed and start at this call's first sample
	WH_CHECK( filterLoopRows( c, batch, FILTER_ARM ) );
	WH_CHECK( enqueueSteps( c, exec, nSteps, nPast + 1, step ) );
	c->lastBatch = batch;
	static_assert( sizeof( wh_token_data ) == sizeof( TokenData ), "token data layout" );
	WH_HIP( hipMemcpyAsync( out, c->greedyOut, sizeof( TokenData ) * (size_t)batch * nSteps, hipMemcpyDeviceToHost, st ) );
	WH_HIP( hipStreamSynchronize( st ) );
	return 0;
}

// Records an event behind everything enqueued for the window so far
static int markWindow( wh_context* c )
{
	hipEvent_t e = nullptr;
	if( !c->markPool.empty() ) { e = c->markPool.back(); c->markPool.pop_back(); }
	else WH_HIP( hipEventCreateWithFlags( &e, hipEventDisableTiming ) );
	WH_HIP( hipEventRecord( e, c->stream ) );
	c->marks.push_back( { c->windowSamples, e } );
	return 0;
}

// Enqueues, without ever blocking the host: prompt step -> first sample (sampleTimestamp rules when requested) -> nSteps
// captured greedy steps. Token data of the 1 + nSteps samples stay on the device until wh_decode_window_finish.
// Several contexts driven this way from one host thread overlap on the GPU (each owns a stream): single-token decode
// steps are latency-bound and use a fraction of the chip, so independent windows fill it concurrently.
static int windowStart( wh_context* c, int batch, const int32_t* promptTokens, const int32_t* promptLens, int nPrompt, int nSteps, int forceFirstTimestamp,
	int firstIsInitial, const char* who )
{
	if( !c || !promptTokens || batch <= 0 || batch > c->maxSeq || ( batch % c->hyp ) != 0 || nPrompt <= 0 || nSteps < 0 ) { setError( "decode_window_start: bad argument" ); return WH_E_INVALIDARG; }
	if( !c->encoded ) { setError( "decode_window_start: wh_encode has not run" ); return WH_E_NOT_READY; }
	WH_BIND( c->m );
	const wh_hparams& hp = c->m->hp;
	if( nPrompt + nSteps > hp.n_text_ctx || (int64_t)batch * nPrompt > c->pinTokenCap() ) { setError( "decode_window_start: too many tokens" ); return WH_E_BOUNDS; }
	bool ragged = false;
	if( promptLens )
		for( int b = 0; b < batch; b++ )
		{
			if( promptLens[ b ] < 1 || promptLens[ b ] > nPrompt ) { setError( "decode_window_start: a prompt length is outside [1, nPromptMax]" ); return WH_E_INVALIDARG; }
			ragged = ragged || promptLens[ b ] != nPrompt;
		}
	if( ragged && c->hyp != 1 ) { setError( "decode_window_start: prompts of different lengths need one hypothesis per window" ); return WH_E_INVALIDARG; }
	// staging: the prompt tokens (padding of a shorter row = token 0: computed, never consumed), the sampler state, the positions
	int32_t* const stTok = c->pinTokens();
	const int M = batch * nPrompt;
	for( int b = 0; b < batch; b++ )
	{
		const int len = promptLens ? promptLens[ b ] : nPrompt;
		WH_CHECK( checkTokens( hp, promptTokens + (size_t)b * nPrompt, len, who ) );
		for( int i = 0; i < nPrompt; i++ ) stTok[ (size_t)b * nPrompt + i ] = i < len ? promptTokens[ (size_t)b * nPrompt + i ] : 0;
	}
	hipStream_t st = c->stream;
	for( auto& mk : c->marks ) c->markPool.push_back( mk.ev );
	c->marks.clear();
	const StepFn step = [ c, batch ]() { return greedyStep( c, batch ); };
	hipGraphExec_t exec = nullptr;
	// no window state exists yet: what the warm-up leaves behind is overwritten below
	if( stepsReplayable( c ) && nSteps > 0 )
		WH_CHECK( obtainStepGraph( c, batch, stepKey( c, 0 ), WARM_FRESH, [ c, batch ]() { return idleLoopState( c, batch ); }, step, exec ) );
	// a new generation per window: stamps of earlier windows in the mailbox can never be taken for this one's
	// (only for the few sequences of a stream whose host loop reads every sample; a lock-step batch is read chunk by chunk through events)
	const bool mailbox = c->mailData && batch <= SMALL_MAX_ROWS;
	if( mailbox ) c->mailCounter = c->mailCounter == 0x7fffffff ? 1 : c->mailCounter + 1;
	c->mailGen = mailbox ? c->mailCounter : 0;
	// after the sampler's advance the position of sequence b must be its prompt length: start one below it
	const DecodeState s0 = { 0, forceFirstTimestamp ? 1 : 0, firstIsInitial ? 1 : 0, c->mailGen };
	{
		int32_t* const stPos = c->pinned + wh_context::PIN_POS;
		for( int b = 0; b < batch; b++ ) stPos[ b ] = ( promptLens ? promptLens[ b ] : nPrompt ) - 1;
		WH_CHECK( uploadDecodeState( c, batch, s0, stPos, 0 ) );
	}
	WH_HIP( hipMemcpyAsync( c->tokensDev, stTok, sizeof( int32_t ) * M, hipMemcpyHostToDevice, st ) );
	c->raggedLastPos = ragged ? c->seqPos : nullptr;
	const int rcGraph = decodeGraph( c, batch, nPrompt, 0, false );
	c->raggedLastPos = nullptr;
	WH_CHECK( rcGraph );
	{
		WH_CHECK( filterLoopRows( c, batch, FILTER_WINDOW ) );	 // a new window: no history survives into it, the prompt does not count, the first sample is unmasked and boosted from the root
		WH_CHECK( sampleStep( c, batch, st ) );
		WH_CHECK( launchAdvanceState( c->state, c->seqPos, batch, st ) );
		c->noSpeechRows = 0;
		if( c->noSpeech )
		{
			// p[ solm ] of the rows the first sample just left in c->probs (the spread sampler leaves unnormalised e and its slice sums), and an event behind it:
			// wh_decode_window_no_speech waits for the first sample only
			WH_CHECK( launchNoSpeechGather( c->probs, spreadSampler( c, batch ) ? c->sampleScratch : nullptr, batch, hp.n_vocab, specialIds( hp ).solm, c->noSpeechDev, st ) );
			WH_HIP( hipEventRecord( c->noSpeechEv, st ) );
			c->noSpeechRows = batch;
		}
	}
	WH_CHECK( enqueueSteps( c, exec, nSteps, nPrompt + 1, step ) );
	c->lastBatch = batch;
	c->windowSamples = 1 + nSteps;
	c->windowPos = nPrompt + nSteps;
	return markWindow( c );
}

int wh_decode_window_start( wh_context* c, int batch, const int32_t* promptTokens, int nPrompt, int nSteps, int forceFirstTimestamp, int firstIsInitial )
{
	return windowStart( c, batch, promptTokens, nullptr, nPrompt, nSteps, forceFirstTimestamp, firstIsInitial, "decode_window_start" );
}

int wh_decode_window_start_ragged( wh_context* c, int batch, const int32_t* promptTokens, const int32_t* promptLens, int nPromptMax, int nSteps,
	int forceFirstTimestamp, int firstIsInitial )
{
	if( !promptLens ) { setError( "decode_window_start_ragged: promptLens is null" ); return WH_E_INVALIDARG; }
	return windowStart( c, batch, promptTokens, promptLens, nPromptMax, nSteps, forceFirstTimestamp, firstIsInitial, "decode_window_start_ragged" );
}

// More greedy steps of the window wh_decode_window_start began, still without blocking the host: the position, the last
// token and the sampler flags live in device memory, so nothing has to come back first. A host loop that looks for a
// stop token keeps one chunk queued behind the one it is reading (wh_decode_window_fetch) and the GPU never idles.
int wh_decode_window_continue( wh_context* c, int nSteps )
{
	if( !c || nSteps <= 0 || c->windowSamples <= 0 ) { setError( "decode_window_continue: no window in progress" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	const wh_hparams& hp = c->m->hp;
	if( c->windowPos + nSteps > hp.n_text_ctx ) { setError( "decode_window_continue: n_text_ctx exceeded" ); return WH_E_BOUNDS; }
	const int batch = c->lastBatch;
	const StepFn step = [ c, batch ]() { return greedyStep( c, batch ); };
	hipGraphExec_t exec = nullptr;
	// a window started with nSteps == 0 captured nothing: the first capture then happens here, over the window's device state
	if( stepsReplayable( c ) ) WH_CHECK( obtainStepGraph( c, batch, stepKey( c, 0 ), WARM_PRESERVE, nullptr, step, exec ) );
	WH_CHECK( enqueueSteps( c, exec, nSteps, c->windowPos + 1, step ) );
	c->windowSamples += nSteps;
	c->windowPos += nSteps;
	return markWindow( c );
}

// Samples [first, first + count) of the window in progress, HOST [count][batch]; blocks only until THOSE samples exist
// (chunks enqueued behind them keep running).
int wh_decode_window_fetch( wh_context* c, int first, int count, wh_token_data* out )
{
	if( !c || !out || first < 0 || count <= 0 || first + count > c->windowSamples ) { setError( "decode_window_fetch: range not enqueued" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	const wh_context::Mark* mk = nullptr;
	for( const auto& x : c->marks )
		if( x.endSample >= first + count ) { mk = &x; break; }
	if( !mk ) { setError( "decode_window_fetch: no completion mark for that range" ); return WH_E_INVALIDARG; }
	if( c->mailData && c->mailGen != 0 && !c->prof.on )
	{
		// the sampler stamps the pinned mailbox after each sample: poll the last stamp of the range (samples are produced in
		// order on one stream, rows of a step by concurrent workgroups: every row of the last step is checked). Nothing is
		// enqueued anywhere -- an event wait + copy + synchronise costs the DECODE stream ~0.2 ms per step (measured, decode1_prof).
		const size_t rows = (size_t)c->lastBatch;
		const volatile int* const flag = c->mailFlag;
		const TokenData* const data = c->mailData + (size_t)first * rows;
		const size_t slot0 = (size_t)first * rows, nRec = rows * (size_t)count;
		const auto t0 = std::chrono::steady_clock::now();
		bool ready = false;
		for( long spins = 0; !ready; spins++ )
		{
			ready = true;
			for( size_t r = 0; r < nRec && ready; r++ ) ready = flag[ 2 * ( slot0 + r ) ] == c->mailGen;
			if( ready )
			{
				// stamped: take the records and hold each against its checksum (a torn or early read fails it: poll on)
				std::atomic_thread_fence( std::memory_order_acquire );
				memcpy( out, data, sizeof( TokenData ) * nRec );
				for( size_t r = 0; r < nRec && ready; r++ )
				{
					TokenData td;
					memcpy( &td, (const char*)out + r * sizeof( TokenData ), sizeof( td ) );
					ready = flag[ 2 * ( slot0 + r ) + 1 ] == sampleChecksum( c->mailGen, td );
				}
				if( ready ) return 0;
			}
			if( ( spins & 255 ) == 255 )
			{
				// a stamp that does not arrive (a driver that does not make the mailbox visible) must not hang the caller;
				// a long wait (the encoder of a window runs ahead of its first sample) does not need a spinning core
				const double waited = std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count();
				if( waited > 0.25 ) break;
				if( waited > 0.002 ) std::this_thread::sleep_for( std::chrono::microseconds( 20 ) );
				else std::this_thread::yield();
			}
		}
	}
	if( !c->copyStream ) WH_HIP( hipStreamCreateWithFlags( &c->copyStream, hipStreamNonBlocking ) );
	WH_HIP( hipStreamWaitEvent( c->copyStream, mk->ev, 0 ) );
	WH_HIP( hipMemcpyAsync( out, c->greedyOut + (size_t)first * c->lastBatch, sizeof( TokenData ) * (size_t)count * c->lastBatch, hipMemcpyDeviceToHost, c->copyStream ) );
	WH_HIP( hipStreamSynchronize( c->copyStream ) );
	return 0;
}

int wh_decode_window_ready( wh_context* c, int first, int count )
{
	if( !c || first < 0 || count <= 0 || first + count > c->windowSamples ) { setError( "decode_window_ready: range not enqueued" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	for( const auto& x : c->marks )
		if( x.endSample >= first + count )
		{
			const hipError_t e = hipEventQuery( x.ev );
			if( e == hipSuccess ) return 1;
			if( e == hipErrorNotReady ) { (void)hipGetLastError(); return 0; }
			return hipFail( e, "hipEventQuery", __FILE__, __LINE__ );
		}
	setError( "decode_window_ready: no completion mark for that range" );
	return WH_E_INVALIDARG;
}

int wh_decode_window_finish( wh_context* c, wh_token_data* out )
{
	if( !c || !out || c->windowSamples <= 0 ) { setError( "decode_window_finish: nothing was started" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	WH_HIP( hipMemcpyAsync( out, c->greedyOut, sizeof( TokenData ) * (size_t)c->lastBatch * c->windowSamples, hipMemcpyDeviceToHost, c->stream ) );
	WH_HIP( hipStreamSynchronize( c->stream ) );
	c->windowSamples = 0;
	return 0;
}

// Temperature sampling for the device-side loop. The factor 1 / T, the seed and the nonce go to device memory, stream-ordered behind what
// is queued; the captured step graph is keyed on the mode only.
int wh_context_set_sampling( wh_context* c, float temperature, uint64_t seed, uint32_t nonce )
{
	if( !c ) { setError( "context_set_sampling: null context" ); return WH_E_INVALIDARG; }
	if( !( temperature >= 0.0f ) || temperature > 4.0f ) { setError( "context_set_sampling: the temperature must lie in [0, 4]" ); return WH_E_INVALIDARG; }
	if( temperature == 0.0f ) { c->temperature = 0.0f; return 0; }
	if( c->hyp != 1 ) { setError( "context_set_sampling: not available on a hypothesis-group context" ); return WH_E_INVALIDARG; }
	if( c->flags & WH_FLAG_PARITY_EXACT ) { setError( "context_set_sampling: not available under WH_FLAG_PARITY_EXACT" ); return WH_E_INVALIDARG; }
	if( c->sampleRowsOn ) { setError( "context_set_sampling: per-row sampling (wh_context_set_sampling_rows) is on" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	if( c->m->hp.n_vocab > SAMPLE_DRAW_MAX_VOCAB ) { setError( "context_set_sampling: vocabulary larger than 65536" ); return WH_E_INVALIDARG; }
	if( !c->sampleParams ) WH_CHECK( c->alloc( c->sampleParams, 1, wh_context::DONT_CARE, "sampleParams" ) );
	const SampleParams p = { 1.0f / temperature, (unsigned)( seed & 0xffffffffull ), (unsigned)( seed >> 32 ), nonce };
	WH_HIP( hipMemcpyAsync( c->sampleParams, &p, sizeof( p ), hipMemcpyHostToDevice, c->stream ) );
	WH_HIP( hipStreamSynchronize( c->stream ) );	 // `p` is on this stack
	c->temperature = temperature;
	return 0;
}

// Per-row sampling for a lock-step batch whose sequences stand at different attempts ("The batch runner"). The records go through pinned
// staging behind what the stream holds -- a chunk queued earlier still reads the old ones -- and the call waits only for the staging's previous upload.
int wh_context_set_sampling_rows( wh_context* c, int rows, const float* temperature, const uint64_t* seed, const uint32_t* nonce )
{
	if( !c || rows < 0 ) { setError( "context_set_sampling_rows: null context or a negative row count" ); return WH_E_INVALIDARG; }
	if( rows == 0 ) { c->sampleRowsOn = 0; return 0; }
	if( !temperature || !seed || !nonce || rows > c->maxSeq ) { setError( "context_set_sampling_rows: null array, or more rows than the context has sequences" ); return WH_E_INVALIDARG; }
	if( c->hyp != 1 ) { setError( "context_set_sampling_rows: not available on a hypothesis-group context" ); return WH_E_INVALIDARG; }
	if( c->flags & WH_FLAG_PARITY_EXACT ) { setError( "context_set_sampling_rows: not available under WH_FLAG_PARITY_EXACT" ); return WH_E_INVALIDARG; }
	if( c->m->hp.n_vocab > SAMPLE_DRAW_MAX_VOCAB ) { setError( "context_set_sampling_rows: vocabulary larger than 65536" ); return WH_E_INVALIDARG; }
	if( c->temperature > 0.0f ) { setError( "context_set_sampling_rows: wh_context_set_sampling has a temperature set" ); return WH_E_INVALIDARG; }
	bool any = false;
	for( int r = 0; r < rows; r++ )
	{
		if( !( temperature[ r ] >= 0.0f ) || temperature[ r ] > 4.0f ) { setError( "context_set_sampling_rows: a temperature lies outside [0, 4]" ); return WH_E_INVALIDARG; }
		any = any || temperature[ r ] > 0.0f;
	}
	// every row greedy: the greedy sampler and its own captured graph, exactly what a context without this call launches
	if( !any ) { c->sampleRowsOn = 0; return 0; }
	WH_BIND( c->m );
	if( !c->sampleRows )
	{
		WH_CHECK( c->alloc( c->sampleRows, (int64_t)c->maxSeq, wh_context::MUST_BE_ZERO, "sampleRows" ) );
		WH_HIP( hipHostMalloc( (void**)&c->sampleRowsPin, sizeof( SampleRowParams ) * (size_t)c->maxSeq, hipHostMallocDefault ) );
		WH_HIP( hipEventCreateWithFlags( &c->sampleRowsEv, hipEventDisableTiming ) );
	}
	else
		WH_HIP( hipEventSynchronize( c->sampleRowsEv ) );	 // the staging's previous upload (long done in a scheduler's round; never the stream's queued work)
	// sequences beyond `rows` are greedy: no record is ever read that was not written
	for( int r = 0; r < c->maxSeq; r++ ) c->sampleRowsPin[ r ] = r < rows ? makeSampleRow( temperature[ r ], seed[ r ], nonce[ r ] ) : makeSampleRow( 0.0f, 0, 0 );
	WH_HIP( hipMemcpyAsync( c->sampleRows, c->sampleRowsPin, sizeof( SampleRowParams ) * (size_t)c->maxSeq, hipMemcpyHostToDevice, c->stream ) );
	WH_HIP( hipEventRecord( c->sampleRowsEv, c->stream ) );
	c->sampleRowsOn = rows;
	return 0;
}

int wh_context_set_no_speech( wh_context* c, int on )
{
	if( !c ) { setError( "context_set_no_speech: null context" ); return WH_E_INVALIDARG; }
	if( on && !c->noSpeechDev )
	{
		WH_BIND( c->m );
		WH_CHECK( c->alloc( c->noSpeechDev, (int64_t)c->maxSeq, wh_context::DONT_CARE, "noSpeech" ) );
		WH_HIP( hipEventCreateWithFlags( &c->noSpeechEv, hipEventDisableTiming ) );
	}
	c->noSpeech = on != 0;
	return 0;
}

int wh_decode_window_no_speech( wh_context* c, float* out )
{
	if( !c || !out || c->noSpeechRows <= 0 ) { setError( "decode_window_no_speech: no window was started with wh_context_set_no_speech on" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	if( !c->copyStream ) WH_HIP( hipStreamCreateWithFlags( &c->copyStream, hipStreamNonBlocking ) );
	WH_HIP( hipStreamWaitEvent( c->copyStream, c->noSpeechEv, 0 ) );
	WH_HIP( hipMemcpyAsync( out, c->noSpeechDev, sizeof( float ) * (size_t)c->noSpeechRows, hipMemcpyDeviceToHost, c->copyStream ) );
	WH_HIP( hipStreamSynchronize( c->copyStream ) );
	return 0;
}

}	// extern "C"
