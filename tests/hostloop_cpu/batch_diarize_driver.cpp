// tests/hostloop_cpu/batch_diarize_driver.cpp -- CPU test harness for stereo diarization in the lock-step batch scheduler (not part of the product).
// One translation unit = the test double of the compute layer (fake_device.cpp) and the batch harness (batch_driver.cpp), both UNCHANGED, plus
//   * an iAudioBuffer that has stereo data (batch_driver.cpp's MemoryBuffer answers nullptr);
//   * bd_run: bt_run over such buffers, with the per-stream speakers in its output (what whisperc_tr_speakers reads from a result) and a new_segment
//     callback that asks the stream's context the way the reference's CLI does (Examples/main/main.cpp:95-118): iContext::detectSpeaker on the times of the
//     new segments, which must be what the results carry for them at that moment.
// diarize.h needs nothing of the compute layer: the library still links with --no-undefined.
#include "fake_device.cpp"
#include "batch_driver.cpp"

namespace
{
	struct StereoBuffer : MemoryBuffer
	{
		std::vector<float> stereo;	  // interleaved, 2 * pcm.size() floats, or empty
		const float* getPcmStereo() const override { return stereo.empty() ? nullptr : stereo.data(); }
	};
	int g_speakerCalls = 0, g_speakerFaults = 0;
	HRESULT newSegmentSpeaker( iContext* ctx, uint32_t nNew, void* ) noexcept
	{
		iTranscribeResult* r = nullptr;
		if( FAILED( ctx->getResults( eResultFlags::Timestamps, &r ) ) || !r ) { g_speakerFaults++; return S_OK; }
		sTranscribeLength len;
		r->getSize( len );
		const ResultData* data = dynamic_cast<const ResultData*>( r );
		if( !data || data->speakers.size() != len.countSegments || len.countSegments < nNew ) { g_speakerFaults++; r->Release(); return S_OK; }
		for( uint32_t i = len.countSegments - nNew; i < len.countSegments; i++ )
		{
			eSpeakerChannel ch = (eSpeakerChannel)0x7E;
			const HRESULT hr = ctx->detectSpeaker( r->getSegments()[ i ].time, ch );
			g_speakerCalls++;
			if( hr != S_OK || (uint8_t)ch != data->speakers[ i ] ) g_speakerFaults++;
		}
		r->Release();
		return S_OK;
	}
	std::string g_diarizeOut;
}

// bt_run's arguments + stereo[b]: nSamples[b] interleaved frames beside pcm[b], or NULL. times[b]: the buffer's media time (iAudioBuffer::getTime).
// bd_result() = {"hr":..,"streams":[{"hr":..,"speakers":[..] or null,"segments":[{"t0","t1"}]}],"speaker_calls":N,"speaker_faults":N}
extern "C" __attribute__( ( visibility( "default" ) ) ) int bd_run( const char* modelPath, uint32_t flags, uint32_t language, const float* const* pcm,
	const float* const* stereo, const int64_t* times, const int32_t* nSamples, int nBuffers, const BatchStreamDesc* streams, int nStreams, uint32_t maxSlots,
	uint32_t groups, int threads )
{
	g_diarizeOut.clear();
	g_speakerCalls = g_speakerFaults = 0;
	g_hostLoopRules = eHostLoopRules::ReferenceCpu;
	std::shared_ptr<LoadedModel> lm = std::make_shared<LoadedModel>();
	HRESULT hr = loadVocabulary( modelPath, lm->vocab );
	if( FAILED( hr ) ) return hr;
	{
		void* w = ref_init( modelPath );
		if( !w ) return E_FAIL;
		int32_t h[ 11 ];
		ref_hparams( w, h );
		ref_free( w );
		lm->hp = wh_hparams{ h[ 0 ], h[ 1 ], h[ 2 ], h[ 3 ], h[ 4 ], h[ 5 ], h[ 6 ], h[ 7 ], h[ 8 ], h[ 9 ], h[ 10 ] };
	}
	lm->gpu = fake_model_create( modelPath, threads );
	TestModel model( lm );
	std::vector<StereoBuffer> buffers( (size_t)nBuffers );
	for( int b = 0; b < nBuffers; b++ )
	{
		buffers[ b ].pcm.assign( pcm[ b ], pcm[ b ] + nSamples[ b ] );
		if( stereo[ b ] ) buffers[ b ].stereo.assign( stereo[ b ], stereo[ b ] + 2 * (size_t)nSamples[ b ] );
		buffers[ b ].time = times[ b ];
	}
	std::vector<sBatchStream> descs( (size_t)nStreams );
	for( int i = 0; i < nStreams; i++ )
		descs[ i ] = sBatchStream{ &buffers[ streams[ i ].buffer ], streams[ i ].firstSample, streams[ i ].countSamples, nullptr };
	sFullParams p{};
	p.strategy = eSamplingStrategy::Greedy;
	p.cpuThreads = threads;
	p.n_max_text_ctx = 16384;
	p.flags = (eFullParamsFlags)flags;
	p.language = language;
	p.thold_pt = p.thold_ptsum = 0.01f;
	p.new_segment_callback = &newSegmentSpeaker;
	const sBatchSetup setup{ maxSlots, groups, 4, 0 };
	iBatchRunner* runner = nullptr;
	hr = createBatchRunner( &model, &setup, &runner );
	if( FAILED( hr ) ) return hr;
	std::vector<iTranscribeResult*> results( (size_t)nStreams, nullptr );
	std::vector<HRESULT> per( (size_t)nStreams, S_OK );
	hr = runner->run( p, descs.data(), (uint32_t)nStreams, results.data(), per.data() );
	std::ostringstream o;
	o << "{\"hr\":" << hr << ",\"streams\":[";
	for( int i = 0; i < nStreams; i++ )
	{
		const ResultData* data = dynamic_cast<const ResultData*>( results[ i ] );
		o << ( i ? "," : "" ) << "{\"hr\":" << per[ i ] << ",\"speakers\":";
		if( data )
		{
			o << "[";
			for( size_t s = 0; s < data->speakers.size(); s++ ) o << ( s ? "," : "" ) << (unsigned)data->speakers[ s ];
			o << "]";
		}
		else
			o << "null";
		o << ",\"segments\":[";
		if( results[ i ] )
		{
			sTranscribeLength len{};
			results[ i ]->getSize( len );
			const sSegment* segs = results[ i ]->getSegments();
			for( uint32_t s = 0; s < len.countSegments; s++ )
				o << ( s ? "," : "" ) << "{\"t0\":" << segs[ s ].time.begin.ticks << ",\"t1\":" << segs[ s ].time.end.ticks << "}";
			results[ i ]->Release();
		}
		o << "]}";
	}
	o << "],\"speaker_calls\":" << g_speakerCalls << ",\"speaker_faults\":" << g_speakerFaults << "}";
	g_diarizeOut = o.str();
	runner->Release();
	return hr;
}
extern "C" __attribute__( ( visibility( "default" ) ) ) const char* bd_result() { return g_diarizeOut.c_str(); }
