// Speech only: the spans of a recording that hold speech, packed one behind the other in device memory, so that the spectrogram -- and with it the encoder
// and the decoder -- sees nothing else (Whisper::setSpeechFilter of whisperApi.h; what faster-whisper calls vad_filter and whisper.cpp --vad). The samples are
// in device memory already when the filter acts (behind the PCM upload, in front of wh_mel_spectrogram*), so no sample makes an extra trip over PCIe:
// 12 bytes per frame go to the host for the decision, a span table comes back.
//
// wh_speech_pack: dst[ out[i] + k ] = src[ a_i + k ] for k < b_i - a_i, out[i] = the spans' lengths summed up to i; FP32 frames of 1 or 2 interleaved
// channels, copied as bits (NaN payloads survive, nothing is converted).
//
// Kernel: a streaming copy, one read and one write per byte, so its bound is the memory system's copy rate (6.3 TB/s for float4 copies on this part) and all
// it can do wrong is issue narrow accesses or too few of them. A workgroup of 256 threads owns SP_SHARE = 16384 consecutive output ELEMENTS (floats: 64 KiB,
// 16 iterations of one 16-byte load and store per thread, unrolled by four so that four loads are in flight per lane before the first store waits; at one
// hour of mono with half of it kept that is 1758 workgroups, 7 per CU). It finds the span its first output lies in with one binary search over the output
// offsets -- the same for every lane: the index depends on blockIdx only -- and walks on from there; a workgroup may cross many short spans. The span rules
// put every a_i and every out[i] on a multiple of 256 samples, so both sides of a span are 16-byte aligned for mono and stereo and the body moves 128-bit
// vectors; only the tail of the last span (b = N, any number) takes single elements. A span whose two sides are NOT both 16-byte aligned (a caller's own
// table, a buffer at an odd address) is copied element by element: correct, at a quarter of the width. No LDS, plain loads and stores, nothing outside
// [0, nOut * channels) of dst.
#include "runtime.h"
#include "../host/speechSpans.h"

namespace wh
{
	namespace
	{
		constexpr int SP_THREADS = 256;
		constexpr long long SP_SHARE = 16384;	   // output elements per workgroup
		constexpr int SP_MAX_SPANS = 65536;
		constexpr int64_t SP_MAX_SAMPLES = (int64_t)1 << 40;

		// table: [count + 1] output offsets, then [count] span starts, in SAMPLES; an element is a float, a sample `channels` of them
		__global__ void __launch_bounds__( SP_THREADS ) speechPackKernel( const float* __restrict__ src, float* __restrict__ dst,
			const long long* __restrict__ table, int count, int channels, long long nOutElems )
		{
			const long long e0 = (long long)blockIdx.x * SP_SHARE;
			if( e0 >= nOutElems ) return;
			const long long e1 = e0 + SP_SHARE < nOutElems ? e0 + SP_SHARE : nOutElems;
			const long long* const outOff = table;
			const long long* const start = table + count + 1;
			// the last span whose first output is at or before e0: out[0] = 0 <= e0 < nOutElems = out[count] * channels
			int lo = 0, hi = count;
			while( hi - lo > 1 )
			{
				const int mid = ( lo + hi ) >> 1;
				if( outOff[ mid ] * channels <= e0 ) lo = mid;
				else hi = mid;
			}
			const int tid = threadIdx.x;
			long long pos = e0;
			for( int i = lo; i < count && pos < e1; i++ )
			{
				const long long spanEnd = outOff[ i + 1 ] * channels;
				const long long end = spanEnd < e1 ? spanEnd : e1;
				if( end <= pos ) continue;
				const float* const s = src + ( start[ i ] - outOff[ i ] ) * channels + pos;	  // the source of output `pos`
				float* const d = dst + pos;
				const long long n = end - pos;
				const bool wide = ( ( (uintptr_t)s | (uintptr_t)d ) & 15 ) == 0;
				const long long nVec = wide ? n >> 2 : 0;
				const float4* const s4 = (const float4*)s;
				float4* const d4 = (float4*)d;
#pragma unroll 4
				for( long long v = tid; v < nVec; v += SP_THREADS ) d4[ v ] = s4[ v ];
				for( long long k = 4 * nVec + tid; k < n; k += SP_THREADS ) d[ k ] = s[ k ];
				pos = end;
			}
		}

		// spans -> the table the kernel reads; false when the spans break the contract
		bool buildTable( const int64_t* spans, int count, int64_t nSamples, int64_t nOut, std::vector<long long>& table )
		{
			table.assign( (size_t)( 2 * count + 1 ), 0 );
			int64_t prevEnd = 0, out = 0;
			for( int i = 0; i < count; i++ )
			{
				const int64_t a = spans[ 2 * i ], b = spans[ 2 * i + 1 ];
				if( a < prevEnd || b <= a || b > nSamples ) return false;
				table[ (size_t)i ] = out;
				table[ (size_t)( count + 1 + i ) ] = a;
				out += b - a;
				prevEnd = b;
			}
			table[ (size_t)count ] = out;
			return out == nOut;
		}

		int launchSpeechPack( hipStream_t stream, const float* src, int channels, const long long* tableDev, int count, float* dst, int64_t nOut )
		{
			const long long elems = nOut * channels;
			const long long blocks = ( elems + SP_SHARE - 1 ) / SP_SHARE;
			if( blocks <= 0 ) return 0;
			if( blocks > 0x7fffffffll ) { setError( "speech_pack: too many outputs for one launch" ); return WH_E_INVALIDARG; }
			hipLaunchKernelGGL( speechPackKernel, dim3( (unsigned)blocks ), dim3( SP_THREADS ), 0, stream, src, dst, tableDev, count, channels, elems );
			WH_HIP( hipGetLastError() );
			return 0;
		}

		bool validCall( const char* who, int channels, int64_t nSamples, const int64_t* spans, int count, int64_t nOut, std::vector<long long>& table )
		{
			if( ( channels != 1 && channels != 2 ) || nSamples < 0 || nSamples > SP_MAX_SAMPLES || count < 0 || count > SP_MAX_SPANS || nOut < 0 || ( count > 0 && !spans ) )
			{
				setError( std::string( who ) + ": 1 or 2 channels, nSamples 0 .. 2^40, 0 .. 65536 spans" );
				return false;
			}
			if( !buildTable( spans, count, nSamples, nOut, table ) )
			{
				setError( std::string( who ) + ": the spans must be non-empty, ascending, disjoint and inside [0, nSamples], and nOut their total length" );
				return false;
			}
			return true;
		}
	}	// namespace
}	// namespace wh

extern "C" {

int wh_speech_pack( void* stream, const float* srcDev, int channels, int64_t nSamples, const int64_t* spans, int count, float* dstDev, int64_t nOut )
{
	std::vector<long long> table;
	if( !validCall( "speech_pack", channels, nSamples, spans, count, nOut, table ) ) return WH_E_INVALIDARG;
	if( count == 0 ) return 0;
	if( !srcDev || !dstDev || ( (uintptr_t)srcDev & 3 ) != 0 || ( (uintptr_t)dstDev & 3 ) != 0 ) { setError( "speech_pack: null or misaligned buffer" ); return WH_E_INVALIDARG; }
	// the table is the call's own: uploaded behind what the stream holds, read by the launch behind it, and the call waits for both before `table` dies
	Allocation t = { nullptr, nullptr, 0, nullptr };
	WH_HIP( guardedAlloc( t, (int64_t)table.size() * 8, -1, "speech spans", (hipStream_t)stream ) );
	hipError_t e = hipMemcpyAsync( t.body, table.data(), table.size() * 8, hipMemcpyHostToDevice, (hipStream_t)stream );
	int rc = 0;
	if( e == hipSuccess ) rc = launchSpeechPack( (hipStream_t)stream, srcDev, channels, (const long long*)t.body, count, dstDev, nOut );
	const hipError_t eSync = hipStreamSynchronize( (hipStream_t)stream );
	if( e == hipSuccess ) e = eSync;
	if( e != hipSuccess ) rc = hipFail( e, "speech_pack", __FILE__, __LINE__ );
	const int bad = guardedFree( t ) > 0;
	if( rc == 0 && bad ) { setError( "speech_pack: a guard region of the span table was written" ); rc = WH_E_BOUNDS; }
	return rc;
}

int wh_speech_pack_host( const float* src, int channels, int64_t nSamples, const int64_t* spans, int count, float* dst, int64_t nOut )
{
	std::vector<long long> table;
	if( !validCall( "speech_pack_host", channels, nSamples, spans, count, nOut, table ) ) return WH_E_INVALIDARG;
	if( count == 0 ) return 0;
	if( !src || !dst ) { setError( "speech_pack_host: null buffer" ); return WH_E_INVALIDARG; }
	Allocation in = { nullptr, nullptr, 0, nullptr }, out = in, t = in;
	hipError_t e = guardedAlloc( in, nSamples * channels * 4, -1, "speech source", nullptr );
	if( e == hipSuccess ) e = guardedAlloc( out, nOut * channels * 4, -1, "speech packed", nullptr );
	if( e == hipSuccess ) e = guardedAlloc( t, (int64_t)table.size() * 8, -1, "speech spans", nullptr );
	int rc = 0;
	if( e == hipSuccess ) e = hipMemcpyAsync( in.body, src, (size_t)( nSamples * channels * 4 ), hipMemcpyHostToDevice, nullptr );
	if( e == hipSuccess ) e = hipMemcpyAsync( t.body, table.data(), table.size() * 8, hipMemcpyHostToDevice, nullptr );
	if( e == hipSuccess ) rc = launchSpeechPack( nullptr, (const float*)in.body, channels, (const long long*)t.body, count, (float*)out.body, nOut );
	if( e == hipSuccess && rc == 0 ) e = hipMemcpyAsync( dst, out.body, (size_t)( nOut * channels * 4 ), hipMemcpyDeviceToHost, nullptr );
	if( e == hipSuccess ) e = hipStreamSynchronize( nullptr );
	if( e != hipSuccess ) rc = hipFail( e, "speech_pack_host", __FILE__, __LINE__ );
	int bad = 0;
	if( in.base ) bad += guardedFree( in ) > 0;
	if( out.base ) bad += guardedFree( out ) > 0;
	if( t.base ) bad += guardedFree( t ) > 0;
	if( rc == 0 && bad ) { setError( "speech_pack_host: a guard region of a device buffer was written" ); rc = WH_E_BOUNDS; }
	return rc;
}

int wh_context_speech_filter( wh_context* c, const float* pcmDev, int64_t nSamples, const float* stereoDev, const wh_speech_params* params,
	const float** packedDev, const float** packedStereoDev, int64_t* nPacked, int64_t* spansOut, int cap, int* count )
{
	if( !c || !packedDev || !nPacked || !count || cap < 0 || ( cap > 0 && !spansOut ) ) { setError( "context_speech_filter: null argument" ); return WH_E_INVALIDARG; }
	WH_BIND( c->m );
	int64_t nFrames = 0;
	if( 0 != wh_vad_frame_count( nSamples, &nFrames ) ) { setError( "context_speech_filter: nSamples 0 .. 2^40" ); return WH_E_INVALIDARG; }
	int64_t minSilence = params ? params->minSilenceFrames : 0, minSpeech = params ? params->minSpeechFrames : 0, pad = params ? params->padFrames : 0;
	if( Whisper::speechRules::resolveParams( minSilence, minSpeech, pad ) < 0 )
	{
		setError( "context_speech_filter: every parameter 0 .. 2^20 frames" );
		return WH_E_INVALIDARG;
	}
	if( nSamples > 0 && ( !pcmDev || ( (uintptr_t)pcmDev & 3 ) != 0 || ( (uintptr_t)stereoDev & 3 ) != 0 ) ) { setError( "context_speech_filter: null or misaligned buffer" ); return WH_E_INVALIDARG; }
	*packedDev = nullptr;
	if( packedStereoDev ) *packedStereoDev = nullptr;
	*nPacked = 0;
	*count = 0;
	// 1. + 2. the features of the whole frames, 12 bytes each, and their way to the host
	std::vector<float> feat( (size_t)nFrames * 3 );
	if( nFrames > 0 )
	{
		WH_CHECK( c->grow( c->speechFeat, nFrames * 3, wh_context::DONT_CARE, "speech features" ) );
		WH_CHECK( wh_vad_features( c->stream, pcmDev, nSamples, c->speechFeat ) );
		WH_HIP( hipMemcpyAsync( feat.data(), c->speechFeat, feat.size() * 4, hipMemcpyDeviceToHost, c->stream ) );
		WH_HIP( hipStreamSynchronize( c->stream ) );
	}
	// 3. the decision and the span rules
	std::vector<uint8_t> speech( (size_t)nFrames );
	Whisper::vad::decide( feat.data(), nFrames, speech.data() );
	std::vector<Whisper::speechRules::Span> spans;
	if( Whisper::speechRules::find( speech.data(), nFrames, nSamples, minSilence, minSpeech, pad, spans ) < 0 )
	{
		setError( "context_speech_filter: the span rules refused the call" );
		return WH_E_INVALIDARG;
	}
	*count = (int)spans.size();
	if( spans.size() > (size_t)SP_MAX_SPANS ) { setError( "context_speech_filter: more than 65536 spans" ); return WH_E_BOUNDS; }
	if( (int)spans.size() > cap ) { setError( "context_speech_filter: the span buffer is too small" ); return WH_E_BOUNDS; }
	std::vector<int64_t> flat;
	for( const auto& s : spans )
	{
		flat.push_back( s.a );
		flat.push_back( s.b );
	}
	if( !flat.empty() ) memcpy( spansOut, flat.data(), flat.size() * 8 );
	const int64_t nOut = Whisper::speechRules::packedLength( spans );
	*nPacked = nOut;
	if( spans.empty() ) return 0;
	// one span that is the whole recording: the packed copy is the recording, nothing is launched
	if( Whisper::speechRules::coversAll( spans, nSamples ) )
	{
		*packedDev = pcmDev;
		if( packedStereoDev ) *packedStereoDev = stereoDev;
		return 0;
	}
	// 4. the table once, the copy for the mono buffer and, if given, the stereo buffer
	std::vector<long long> table;
	if( !buildTable( flat.data(), (int)spans.size(), nSamples, nOut, table ) ) { setError( "context_speech_filter: internal error (span table)" ); return WH_E_BOUNDS; }
	WH_CHECK( c->grow( c->speechTable, (int64_t)table.size(), wh_context::DONT_CARE, "speech spans" ) );
	WH_CHECK( c->grow( c->speechMono, nOut, wh_context::DONT_CARE, "speech packed mono" ) );
	if( stereoDev ) WH_CHECK( c->grow( c->speechStereo, nOut * 2, wh_context::DONT_CARE, "speech packed stereo" ) );
	WH_HIP( hipMemcpyAsync( c->speechTable, table.data(), table.size() * 8, hipMemcpyHostToDevice, c->stream ) );
	int rc = launchSpeechPack( c->stream, pcmDev, 1, c->speechTable, (int)spans.size(), c->speechMono, nOut );
	if( rc == 0 && stereoDev ) rc = launchSpeechPack( c->stream, stereoDev, 2, c->speechTable, (int)spans.size(), c->speechStereo, nOut );
	// `table` dies with this call
	const hipError_t e = hipStreamSynchronize( c->stream );
	if( rc != 0 ) return rc;
	if( e != hipSuccess ) return hipFail( e, "context_speech_filter", __FILE__, __LINE__ );
	*packedDev = c->speechMono;
	if( packedStereoDev ) *packedStereoDev = stereoDev ? c->speechStereo : nullptr;
	return 0;
}

}	// extern "C"
