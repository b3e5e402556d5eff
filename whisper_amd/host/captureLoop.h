// The loop of iContext::runCapture: Capture::run of the reference restated (Whisper/Whisper/ContextImpl.capture.cpp:212-288) with its state word (:95-123),
// its parameters (:53-69, :403-416) and postPoolWork (:134-147). Host only, no device, no other header of this library than the API's and vad.h:
// tests/capture_cpu/driver.cpp compiles it alone. What touches a device or a thread is injected (Hooks): reading a chunk into the buffer, the voice-activity
// step over the frames a read completed, handing the buffer to the transcription job, and the two questions about that job. capture.cpp supplies them.
//
// Departures from the reference, each needed because the source is a pipe or the caller's code and not a sound card:
//   1. End of stream. The reference's devices never end (readSample answers E_EOF, :311-312, and runCapture fails with it). Here a closed and drained
//      source ends the loop: it waits for the running job, posts what is buffered if the last voice-activity answer was not 0, waits for that job and
//      returns S_OK.
//   2. eCaptureFlags::NoDrop. Wherever the loop would post and the job is busy (:278-287) it waits for the job and posts, instead of growing the buffer and
//      stalling: no sample is ever discarded, and the pieces depend on the audio and the chunk sizes only, not on timing.
//   3. Under NoDrop the Transcribing bit is cleared by the thread that runs the loop, where it waits for the job anyway, so that the sequence of status
//      words is a function of the audio and the chunk sizes too. Without NoDrop it is the reference's: whoever runs the job calls workerEnded() when it
//      ends (workCallback, :360-365) and the bit falls then, from that thread; the loop only collects the job's result before its next read. (A caller of
//      this header that never calls workerEnded(), like the scripted driver of the tests, sees the bit fall at that collection.)
#pragma once
#include "whisperApi.h"
#include "vad.h"
#include <atomic>
#include <cmath>
#include <cstdint>
#include <functional>

namespace Whisper
{
	namespace captureLoop
	{
		constexpr int64_t SAMPLE_RATE = 16000;
		constexpr uint8_t LISTENING = (uint8_t)eCaptureStatus::Listening, VOICE = (uint8_t)eCaptureStatus::Voice, TRANSCRIBING = (uint8_t)eCaptureStatus::Transcribing,
						  STALLED = (uint8_t)eCaptureStatus::Stalled;

		// seconds -> samples: the product in FP32, rounded to the nearest integer, ties to even (:58-65: _mm_mul_ps, _mm_round_ps( NINT ), _mm_cvtps_epi32)
		inline uint32_t samplesFromSeconds( float seconds )
		{
			const float v = seconds * (float)SAMPLE_RATE;
			// the reference converts whatever it is given; what no uint32 of samples can mean is held here: NaN and negative count as 0, the top is 2^30
			if( !( v > 0.0f ) ) return 0;
			if( v >= 1073741824.0f ) return 1073741824u;
			// nearbyint under the default rounding mode; stated by hand so that no rounding mode set elsewhere changes it
			const float f = std::floor( v );
			const float d = v - f;	  // exact (above 2^23 every float is an integer: d = 0)
			float r = f;
			if( d > 0.5f || ( d == 0.5f && std::fmod( f, 2.0f ) != 0.0f ) ) r = f + 1.0f;
			return (uint32_t)(int32_t)r;
		}

		// CaptureParams (:53-69): the durations in samples
		struct Params
		{
			uint32_t minDuration = 0, maxDuration = 0, dropStartSilence = 0, pauseDuration = 0, flags = 0;
			Params() = default;
			explicit Params( const sCaptureParams& cp )
				: minDuration( samplesFromSeconds( cp.minDuration ) ), maxDuration( samplesFromSeconds( cp.maxDuration ) ),
				  dropStartSilence( samplesFromSeconds( cp.dropStartSilence ) ), pauseDuration( samplesFromSeconds( cp.pauseDuration ) ), flags( cp.flags )
			{
			}
			bool noDrop() const { return 0 != ( flags & (uint32_t)eCaptureFlags::NoDrop ); }
		};

		// runCapture's checks (:403-416); *which (optional) names the parameter that is out of range. `!( a >= b && a <= c )` so that a NaN is refused.
		inline HRESULT validate( const sCaptureParams& cp, const char** which = nullptr )
		{
			if( !( cp.minDuration >= 0.125f && cp.minDuration <= 30.0f ) ) { if( which ) *which = "minDuration"; return E_INVALIDARG; }
			if( !( cp.maxDuration >= 0.125f && cp.maxDuration <= 30.0f ) ) { if( which ) *which = "maxDuration"; return E_INVALIDARG; }
			return S_OK;
		}

		// the buffer's media time (:34-38, MFllMulDiv( currentOffset, 10'000'000, SAMPLE_RATE, 0 )): 625 ticks of 100 ns per sample
		inline int64_t ticksFromSamples( int64_t samples ) { return samples * 10000000ll / SAMPLE_RATE; }

		struct Hooks
		{
			// callbacks.shouldCancel (:171-176): anything but S_OK ends the loop; a failure is the loop's result
			std::function<HRESULT()> shouldCancel;
			// callbacks.captureStatus with the new state word, called only when a bit changed
			std::function<HRESULT( uint8_t )> status;
			// readSample (:290-358): the next chunk, appended to the buffer, or only counted when `discard`. frames: its sample frames. feat / newFrames: the
			// features of the 256-sample frames of the BUFFER that this chunk completed (nothing when discarded). S_FALSE: the stream has ended, nothing was read.
			std::function<HRESULT( bool discard, uint32_t& frames, const float*& feat, int64_t& newFrames )> read;
			// detectVoice (:391-395) made incremental: the features of the new frames and the size of the buffer behind the read -> lastVoice, the end of the
			// last speech frame of the whole buffer in samples, 0 for none. vadClear: VAD::clear. DetectorStep below is the real one; a test may script it.
			std::function<int64_t( const float* feat, int64_t newFrames, int64_t bufferSamples )> vadStep;
			std::function<void()> vadClear;
			// pcm.clear() (:245): empties the buffer without handing it to anybody
			std::function<void()> dropBuffer;
			// postPoolWork's middle (:139-142): hands the buffer over -- it begins at sample `start` of the stream and holds `count` samples -- and starts the job;
			// the buffer is empty afterwards
			std::function<HRESULT( int64_t start, int64_t count )> post;
			// workStatus (:81, :270-276) of the job posted last: S_OK it has ended well, S_FALSE it runs, a failure is its result. jobWait blocks until it has ended.
			std::function<HRESULT()> jobPoll, jobWait;
		};

		// The voice-activity step over vad::Detector, with detect's rule for a buffer of less than one frame (voiceActivityDetection.cpp:124-129)
		struct DetectorStep
		{
			vad::Detector d;
			// speech (may be nullptr): one byte per fed frame
			int64_t step( const float* feat, int64_t newFrames, int64_t bufferSamples, uint8_t* speech = nullptr )
			{
				if( bufferSamples / vad::FRAME_SAMPLES <= 0 )
				{
					d.clear();
					return 0;
				}
				return d.feed( feat, newFrames, speech );
			}
			void clear() { d.clear(); }
		};

		class Loop
		{
			const Params p;
			const Hooks h;
			std::atomic<uint8_t> state{ 0 };	  // InterlockedOr8 / InterlockedAnd8 of the reference: the worker clears Transcribing
			bool jobPending = false;			  // a job was posted and its result not collected yet (the reference's workStatus == S_FALSE, seen from the loop)
			int64_t bufferSamples = 0;
			int64_t pcmStartTime = 0, nextSampleTime = 0;
			int64_t lastVoice = 0;

			// setStateFlag / clearStateFlag (:95-117)
			HRESULT setFlag( uint8_t bit )
			{
				const uint8_t old = state.fetch_or( bit );
				if( !h.status || 0 != ( old & bit ) ) return S_OK;
				return h.status( (uint8_t)( old | bit ) );
			}
			HRESULT clearFlag( uint8_t bit )
			{
				const uint8_t old = state.fetch_and( (uint8_t)~bit );
				if( !h.status || 0 == ( old & bit ) ) return S_OK;
				return h.status( (uint8_t)( old & (uint8_t)~bit ) );
			}
			bool has( uint8_t bit ) const { return 0 != ( state.load() & bit ); }

			// postPoolWork (:134-147)
			HRESULT post()
			{
				HRESULT hr = setFlag( TRANSCRIBING );
				if( FAILED( hr ) ) return hr;
				jobPending = true;
				hr = h.post( pcmStartTime, bufferSamples );
				if( FAILED( hr ) ) { jobPending = false; return hr; }
				pcmStartTime = nextSampleTime;
				bufferSamples = 0;
				lastVoice = 0;
				h.vadClear();
				return S_OK;
			}
			// the job's result is in: the bit falls here unless workerEnded() cleared it already; the job's failure is the loop's
			HRESULT jobEnded( HRESULT jobResult )
			{
				jobPending = false;
				const HRESULT hr = clearFlag( TRANSCRIBING );
				return FAILED( jobResult ) ? jobResult : hr;
			}
			HRESULT waitForJob()
			{
				if( !jobPending ) return S_OK;
				return jobEnded( h.jobWait() );
			}

			// one pass of Capture::run (:212-288). S_FALSE: the stream has ended.
			HRESULT step()
			{
				HRESULT hr;
				if( !p.noDrop() && jobPending )
				{
					hr = h.jobPoll();
					if( hr != S_FALSE )
					{
						hr = jobEnded( hr );
						if( FAILED( hr ) ) return hr;
					}
				}
				uint32_t frames = 0;
				const float* feat = nullptr;
				int64_t newFrames = 0;
				if( has( STALLED ) )
				{
					if( jobPending )
					{
						// :221-222 still stalled: the read is discarded, the sample clock goes on (:340-343)
						hr = h.read( true, frames, feat, newFrames );
						if( hr != S_OK ) return hr;
						nextSampleTime += frames;
						return S_OK;
					}
					// :226-229 the postponed job has ended: no longer stalled, the buffer goes to the job; nothing is read in this pass
					hr = clearFlag( STALLED );
					if( FAILED( hr ) ) return hr;
					return post();
				}

				const int64_t oldSamples = bufferSamples;	 // :233-235
				hr = h.read( false, frames, feat, newFrames );
				if( hr != S_OK ) return hr;
				bufferSamples += frames;
				nextSampleTime += frames;	 // :335-338
				const int64_t newSamples = bufferSamples;

				lastVoice = h.vadStep( feat, newFrames, bufferSamples );	  // :237
				if( lastVoice == 0 )
				{
					// :240-248 no voice in the whole buffer
					clearFlag( VOICE );	   // the reference does not look at these results (:241, :256, :263, :286)
					if( newSamples < (int64_t)p.dropStartSilence ) return S_OK;
					h.dropBuffer();
					bufferSamples = 0;
					h.vadClear();
					pcmStartTime = nextSampleTime;
					return S_OK;
				}

				const bool newFrameVoice = lastVoice + (int64_t)p.pauseDuration >= oldSamples;	   // :251 old, not new
				if( newFrameVoice )
				{
					// :253-259 voice, and fairly recently: grow up to maxDuration
					setFlag( VOICE );
					if( newSamples < (int64_t)p.maxDuration ) return S_OK;
				}
				else
				{
					// :260-266 voice, but a while ago: fire once minDuration is there
					clearFlag( VOICE );
					if( newSamples < (int64_t)p.minDuration ) return S_OK;
				}

				// :268-276
				if( !jobPending ) return post();
				if( p.noDrop() )
				{
					// departure 2
					hr = waitForJob();
					if( FAILED( hr ) ) return hr;
					return post();
				}
				// :278-287 the job still runs: grow up to maxDuration, then drop what comes
				if( newSamples < (int64_t)p.maxDuration ) return S_OK;
				setFlag( STALLED );
				return S_OK;
			}

		public:
			Loop( const Params& params, const Hooks& hooks ) : p( params ), h( hooks ) {}

			uint8_t stateWord() const { return state.load(); }

			// workCallback's second line (:363), for whoever runs the job, from its own thread, when the job has ended -- not under NoDrop (departure 3)
			void workerEnded()
			{
				if( !p.noDrop() ) clearFlag( TRANSCRIBING );
			}

			// startup's last line (:207) and the loop of runCapture (:422-429); a running job is waited for before returning (the reference: ~Capture, :157-161)
			HRESULT run()
			{
				HRESULT res = setFlag( LISTENING );
				bool ended = false;
				while( SUCCEEDED( res ) )
				{
					if( h.shouldCancel )
					{
						const HRESULT hr = h.shouldCancel();
						if( FAILED( hr ) ) { res = hr; break; }
						if( hr != S_OK ) break;
					}
					res = step();
					if( res == S_FALSE ) { ended = true; res = S_OK; break; }
				}
				const HRESULT hrJob = waitForJob();
				if( SUCCEEDED( res ) ) res = FAILED( hrJob ) ? hrJob : S_OK;
				if( ended && SUCCEEDED( res ) )
				{
					// departure 1
					res = clearFlag( STALLED );
					if( SUCCEEDED( res ) && bufferSamples > 0 && lastVoice != 0 )
					{
						res = post();
						if( SUCCEEDED( res ) ) res = waitForJob();
					}
				}
				return FAILED( res ) ? res : S_OK;
			}
		};
	}
}
