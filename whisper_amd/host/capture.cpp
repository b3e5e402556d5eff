// Live transcription: iContext::runCapture over an iPcmCapture (whisperApi.h). The loop is captureLoop.h's -- Capture::run of the reference
// (Whisper/Whisper/ContextImpl.capture.cpp) --; this unit supplies what the loop leaves open: the source (a queue of chunks the caller writes from any
// thread), the buffer (wh_capture of whisper_hip.h: one launch per chunk converts it and gives the voice-activity features of the frames it completes), and
// the job (iContext::runFull of the piece's host mirror on a worker thread, media time = the piece's first sample).
//
// A capture at another rate than 16 kHz (createPcmCaptureAtRate) is resampled by the buffer, chunk by chunk: what a read appends is then not the chunk's frame
// count but the 16 kHz samples the device reports, possibly none (the filter looks half + 1 input frames ahead); a discarded read moves the stream's output
// clock (skip) without an upload; and the end of the stream is one last read, the flush. The loop counts 16 kHz samples as before, so a piece's start is an
// index into the whole stream's resampled output. The three device entries this needs are reached through captureRate.h's table.
#include "hostCommon.h"
#include "captureLoop.h"
#include "captureRate.h"
#include <algorithm>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>

namespace Whisper
{
	namespace
	{
		// a queued chunk is at most a second of input: the capture buffer is sized 30 s plus one chunk
		constexpr uint32_t MAX_CHUNK_FRAMES = 16000;
		constexpr int64_t CAP_SAMPLES = 30 * captureLoop::SAMPLE_RATE + MAX_CHUNK_FRAMES;
		// at another rate a second of input is 16000 outputs or one more, and the flush adds the look-ahead's (at most 35 * 16 + 1)
		constexpr int64_t CAP_SAMPLES_RATE = CAP_SAMPLES + 1024;

		struct Chunk
		{
			std::vector<uint8_t> bytes;
			uint32_t frames = 0;
		};

		// what runCapture needs from a capture of this library
		// {c4b1d6e0-92a7-4e35-8f1c-5d3a7b9e2f64}
		struct iPcmQueue : public ComLight::IUnknown
		{
			static constexpr ComLight::GUID iid() { return { 0xc4b1d6e0, 0x92a7, 0x4e35, { 0x8f, 0x1c, 0x5d, 0x3a, 0x7b, 0x9e, 0x2f, 0x64 } }; }
			// a loop drains the queue from now on (write may block under NoDrop) / no longer does. E_UNEXPECTED when another loop already does.
			virtual HRESULT attach() = 0;
			virtual void detach() = 0;
			// waits for the next chunk; false: the stream was closed and the queue is empty
			virtual bool pop( Chunk& c, int& format, int& channels ) = 0;
			// frames per second of what is written
			virtual uint32_t sampleRate() const = 0;
		};

		class PcmCapture : public iPcmCapture, public iPcmQueue
		{
			std::atomic<uint32_t> rc{ 1 };
			const sCaptureParams params;
			const uint32_t rate;
			const int64_t limitFrames;	   // maxDuration + 1 s, in input frames
			mutable std::mutex mx;
			std::condition_variable cvData, cvSpace;
			std::deque<Chunk> queue;
			int64_t queuedFrames = 0;
			uint64_t dropped = 0;
			int format = -1, channels = 0;
			bool closed = false, attached = false;

			static int64_t limitOf( const sCaptureParams& p, uint32_t rate )
			{
				const float seconds = p.maxDuration > 0 && p.maxDuration <= 30.0f ? p.maxDuration : 30.0f;
				if( rate == captureLoop::SAMPLE_RATE ) return (int64_t)captureLoop::samplesFromSeconds( seconds ) + captureLoop::SAMPLE_RATE;
				return (int64_t)( (double)seconds * (double)rate + 0.5 ) + (int64_t)rate;
			}

		public:
			PcmCapture( const sCaptureParams& p, uint32_t sampleRate ) : params( p ), rate( sampleRate ), limitFrames( limitOf( p, sampleRate ) ) {}
			virtual ~PcmCapture() = default;
			HRESULT QueryInterface( const ComLight::GUID& riid, void** ppv ) override
			{
				if( !ppv ) return E_POINTER;
				if( riid == iPcmCapture::iid() || riid == iAudioCapture::iid() || riid == ComLight::IID_IUnknown ) { *ppv = static_cast<iPcmCapture*>( this ); AddRef(); return S_OK; }
				if( riid == iPcmQueue::iid() ) { *ppv = static_cast<iPcmQueue*>( this ); AddRef(); return S_OK; }
				*ppv = nullptr;
				return E_NOINTERFACE;
			}
			uint32_t AddRef() override { return ++rc; }
			uint32_t Release() override
			{
				const uint32_t r = --rc;
				if( r == 0 ) delete this;
				return r;
			}
			// no Media Foundation here, like the WAV reader's
			HRESULT getReader( IMFSourceReader** pp ) const override { if( pp ) *pp = nullptr; return E_NOTIMPL; }
			const sCaptureParams& getParams() const override { return params; }

			HRESULT write( const void* samples, int fmt, int ch, uint32_t frames ) override
			{
				if( fmt != WH_PCM_S16 && fmt != WH_PCM_F32 ) { logError( "iPcmCapture.write: the format must be 1 (s16) or 4 (f32)" ); return E_INVALIDARG; }
				if( ch != 1 && ch != 2 ) { logError( "iPcmCapture.write: 1 or 2 channels" ); return E_INVALIDARG; }
				if( frames == 0 ) return S_OK;
				if( !samples ) return E_POINTER;
				const size_t frameBytes = (size_t)ch * ( fmt == WH_PCM_S16 ? 2 : 4 );
				std::unique_lock<std::mutex> lk( mx );
				if( closed ) return E_UNEXPECTED;
				if( format < 0 ) { format = fmt; channels = ch; }
				else if( format != fmt || channels != ch ) { logError( "iPcmCapture.write: the format and the channel count of a capture do not change" ); return E_INVALIDARG; }
				const bool noDrop = 0 != ( params.flags & (uint32_t)eCaptureFlags::NoDrop );
				for( uint32_t done = 0; done < frames; )
				{
					const uint32_t n = std::min( frames - done, rate );	   // MAX_CHUNK_FRAMES at 16 kHz
					if( noDrop )
					{
						// with no loop attached nobody would ever make room: the queue grows
						cvSpace.wait( lk, [ & ] { return !attached || queuedFrames <= limitFrames || closed; } );
						if( closed ) return E_UNEXPECTED;
					}
					else
						while( queuedFrames > limitFrames && !queue.empty() )
						{
							queuedFrames -= queue.front().frames;
							queue.pop_front();
							dropped++;
						}
					Chunk c;
					c.frames = n;
					const uint8_t* src = (const uint8_t*)samples + (size_t)done * frameBytes;
					c.bytes.assign( src, src + (size_t)n * frameBytes );
					queue.push_back( std::move( c ) );
					queuedFrames += n;
					done += n;
					cvData.notify_one();
				}
				return S_OK;
			}
			HRESULT close() override
			{
				std::lock_guard<std::mutex> lk( mx );
				closed = true;
				cvData.notify_all();
				cvSpace.notify_all();
				return S_OK;
			}
			uint64_t droppedChunks() const override
			{
				std::lock_guard<std::mutex> lk( mx );
				return dropped;
			}

			HRESULT attach() override
			{
				std::lock_guard<std::mutex> lk( mx );
				if( attached ) return E_UNEXPECTED;
				attached = true;
				return S_OK;
			}
			void detach() override
			{
				std::lock_guard<std::mutex> lk( mx );
				attached = false;
				cvSpace.notify_all();
			}
			bool pop( Chunk& c, int& fmt, int& ch ) override
			{
				std::unique_lock<std::mutex> lk( mx );
				cvData.wait( lk, [ & ] { return !queue.empty() || closed; } );
				if( queue.empty() ) return false;
				c = std::move( queue.front() );
				queue.pop_front();
				queuedFrames -= c.frames;
				fmt = format;
				ch = channels;
				cvSpace.notify_all();
				return true;
			}
			uint32_t sampleRate() const override { return rate; }
		};

		// TranscribeBuffer (ContextImpl.capture.cpp:15-42) over the host mirror wh_capture_take handed out; lives on runCapture's stack
		class PieceBuffer : public iAudioBuffer
		{
		public:
			const float *mono = nullptr, *stereo = nullptr;
			uint32_t count = 0;
			int64_t startSample = 0;
			HRESULT QueryInterface( const ComLight::GUID& riid, void** ppv ) override
			{
				if( !ppv ) return E_POINTER;
				if( riid == iAudioBuffer::iid() || riid == ComLight::IID_IUnknown ) { *ppv = static_cast<iAudioBuffer*>( this ); return S_OK; }
				*ppv = nullptr;
				return E_NOINTERFACE;
			}
			uint32_t AddRef() override { return 2; }
			uint32_t Release() override { return 1; }
			uint32_t countSamples() const override { return count; }
			const float* getPcmMono() const override { return count ? mono : nullptr; }
			const float* getPcmStereo() const override { return count ? stereo : nullptr; }
			HRESULT getTime( int64_t& rdi ) const override { rdi = captureLoop::ticksFromSamples( startSample ); return S_OK; }
		};

		// the session: the device buffer, the worker and the hooks of the loop
		struct Session
		{
			iContext* const context;
			wh_context* const gpu;
			const sFullParams& fullParams;
			const sCaptureCallbacks& callbacks;
			iPcmQueue* const source;
			const bool keepStereo;
			const uint32_t rate;
			const CaptureRateTable* const table;	// non-null when rate is not 16000
			pfnCapturePiece const pfnPiece;
			void* const pvPiece;

			wh_capture* cap = nullptr;
			captureLoop::Loop* loop = nullptr;	   // told when a job ends (workerEnded)
			bool ended = false;					   // at another rate: the end of the stream was answered with the flush
			std::vector<float> feat;
			captureLoop::DetectorStep detector;
			PieceBuffer buffer;
			std::thread worker;
			std::atomic<bool> jobDone{ true };
			HRESULT jobResult = S_OK;

			Session( iContext* c, wh_context* g, const sFullParams& fp, const sCaptureCallbacks& cb, iPcmQueue* q, bool st, const CaptureRateTable* t, pfnCapturePiece pfn, void* pv )
				: context( c ), gpu( g ), fullParams( fp ), callbacks( cb ), source( q ), keepStereo( st ), rate( q->sampleRate() ), table( t ), pfnPiece( pfn ), pvPiece( pv )
			{
			}
			~Session()
			{
				if( worker.joinable() ) worker.join();
				if( cap ) wh_capture_destroy( cap );
			}

			// frames: the 16 kHz samples the read appended to the buffer or, when discarded, moved the stream's clock by
			HRESULT read( bool discard, uint32_t& frames, const float*& features, int64_t& newFrames )
			{
				if( rate != captureLoop::SAMPLE_RATE ) return readAtRate( discard, frames, features, newFrames );
				Chunk c;
				int format = 0, channels = 0;
				frames = 0;
				features = nullptr;
				newFrames = 0;
				if( !source->pop( c, format, channels ) ) return S_FALSE;
				frames = c.frames;
				if( discard ) return S_OK;
				// the buffer is made for the stream's channel count, which the first chunk tells
				if( !cap ) CHECK_WH( wh_capture_create( gpu, channels, keepStereo ? 1 : 0, CAP_SAMPLES, &cap ) );
				feat.resize( (size_t)( c.frames / vad::FRAME_SAMPLES + 1 ) * 3 );
				CHECK_WH( wh_capture_append( cap, c.bytes.data(), format, c.frames, feat.data(), (int64_t)feat.size() / 3, &newFrames ) );
				features = feat.data();
				return S_OK;
			}
			HRESULT readAtRate( bool discard, uint32_t& frames, const float*& features, int64_t& newFrames )
			{
				Chunk c;
				int format = 0, channels = 0;
				frames = 0;
				features = nullptr;
				newFrames = 0;
				if( ended ) return S_FALSE;
				int64_t before = 0, after = 0, grown = 0;
				if( !source->pop( c, format, channels ) )
				{
					// the end of the stream is one last read: the outputs whose taps reach past the last frame. S_FALSE to the read after it.
					ended = true;
					if( !cap ) return S_FALSE;
					if( discard )
					{
						CHECK_WH( table->skip( cap, 0, &grown ) );
						frames = (uint32_t)grown;
						return S_OK;
					}
					feat.resize( 8 * 3 );
					CHECK_WH( wh_capture_size( cap, &before ) );
					CHECK_WH( table->flush( cap, feat.data(), (int64_t)feat.size() / 3, &newFrames ) );
					CHECK_WH( wh_capture_size( cap, &after ) );
					frames = (uint32_t)( after - before );
					features = feat.data();
					return S_OK;
				}
				if( !cap ) CHECK_WH( table->createRate( gpu, channels, keepStereo ? 1 : 0, CAP_SAMPLES_RATE, (int)rate, &cap ) );
				if( discard )
				{
					// nothing is uploaded: the stream counts the frames, and what follows is filtered as if they had been zeros
					CHECK_WH( table->skip( cap, c.frames, &grown ) );
					frames = (uint32_t)grown;
					return S_OK;
				}
				// the chunk makes at most ceil( frames 16000 / rate ) + 1 outputs ready
				const int64_t mostOutputs = ( (int64_t)c.frames * captureLoop::SAMPLE_RATE + rate - 1 ) / rate + 1;
				feat.resize( (size_t)( mostOutputs / vad::FRAME_SAMPLES + 1 ) * 3 );
				CHECK_WH( wh_capture_size( cap, &before ) );
				CHECK_WH( wh_capture_append( cap, c.bytes.data(), format, c.frames, feat.data(), (int64_t)feat.size() / 3, &newFrames ) );
				CHECK_WH( wh_capture_size( cap, &after ) );
				frames = (uint32_t)( after - before );
				features = feat.data();
				return S_OK;
			}
			HRESULT post( int64_t start, int64_t count )
			{
				if( worker.joinable() ) worker.join();	  // the loop posts only behind a job that has ended
				int64_t n = 0;
				CHECK_WH( wh_capture_take( cap, &buffer.mono, &buffer.stereo, &n ) );
				if( n != count ) return E_UNEXPECTED;
				buffer.count = (uint32_t)n;
				buffer.startSample = start;
				jobDone = false;
				worker = std::thread( [ this ]() {
					// workCallback (:360-365); a failure of runFull is the job's result
					HRESULT hr = context->runFull( fullParams, &buffer );
					if( SUCCEEDED( hr ) && pfnPiece ) pfnPiece( pvPiece, buffer.startSample, (int64_t)buffer.count );
					jobResult = FAILED( hr ) ? hr : S_OK;
					if( loop ) loop->workerEnded();	   // :363 the Transcribing bit falls when the job ends, from this thread (not under NoDrop)
					jobDone = true;
				} );
				return S_OK;
			}
			HRESULT jobPoll()
			{
				if( !jobDone ) return S_FALSE;
				return jobWait();
			}
			HRESULT jobWait()
			{
				if( worker.joinable() ) worker.join();
				return jobResult;
			}
		};
	}

	const CaptureRateTable* g_captureRateTable = nullptr;

	HRESULT createPcmCaptureAtRate( const sCaptureParams& params, uint32_t sampleRate, iPcmCapture** pp )
	{
		if( !pp ) return E_POINTER;
		*pp = nullptr;
		if( sampleRate < CAPTURE_MIN_RATE || sampleRate > CAPTURE_MAX_RATE )
		{
			logError( "createPcmCaptureAtRate: the sample rate must be 1000 .. 384000 Hz" );
			return E_INVALIDARG;
		}
		*pp = new PcmCapture( params, sampleRate );
		return S_OK;
	}
	HRESULT createPcmCapture( const sCaptureParams& params, iPcmCapture** pp )
	{
		return createPcmCaptureAtRate( params, (uint32_t)captureLoop::SAMPLE_RATE, pp );
	}

	HRESULT runCaptureLoop( iContext* context, wh_context* gpu, const sFullParams& params, const sCaptureCallbacks& callbacks, const iAudioCapture* reader,
		pfnCapturePiece pfnPiece, void* pvPiece )
	{
		if( !reader ) return E_POINTER;
		if( !context || !gpu ) return E_UNEXPECTED;
		iPcmQueue* source = nullptr;
		if( FAILED( const_cast<iAudioCapture*>( reader )->QueryInterface( iPcmQueue::iid(), (void**)&source ) ) || !source )
		{
			logError( "runCapture: this capture was not created by Whisper::createPcmCapture of this library" );
			return E_INVALIDARG;
		}
		struct Detach
		{
			iPcmQueue* q;
			bool attached = false;
			~Detach() { if( attached ) q->detach(); q->Release(); }
		} guard{ source };

		// :403-416
		const sCaptureParams& cp = reader->getParams();
		const char* which = nullptr;
		if( FAILED( captureLoop::validate( cp, &which ) ) )
		{
			logError( "%s parameter %g is out of range", which, which[ 1 ] == 'i' ? cp.minDuration : cp.maxDuration );
			return E_INVALIDARG;
		}
		const CaptureRateTable* const table = g_captureRateTable;
		if( source->sampleRate() != captureLoop::SAMPLE_RATE && !table )
		{
			logError( "runCapture: a capture at a sample rate of %u Hz needs the device resampler, which this build of the library does not install", source->sampleRate() );
			return E_NOTIMPL;
		}
		CHECK( source->attach() );
		guard.attached = true;

		Session s( context, gpu, params, callbacks, source, 0 != ( cp.flags & (uint32_t)eCaptureFlags::Stereo ), table, pfnPiece, pvPiece );
		captureLoop::Hooks h;
		if( callbacks.shouldCancel ) h.shouldCancel = [ & ]() { return callbacks.shouldCancel( callbacks.pv ); };
		if( callbacks.captureStatus ) h.status = [ & ]( uint8_t word ) { return callbacks.captureStatus( callbacks.pv, (eCaptureStatus)word ); };
		h.read = [ & ]( bool discard, uint32_t& frames, const float*& feat, int64_t& newFrames ) { return s.read( discard, frames, feat, newFrames ); };
		h.vadStep = [ & ]( const float* feat, int64_t newFrames, int64_t bufferSamples ) { return s.detector.step( feat, newFrames, bufferSamples ); };
		h.vadClear = [ & ]() { s.detector.clear(); };
		h.dropBuffer = [ & ]() { if( s.cap ) wh_capture_clear( s.cap ); };
		h.post = [ & ]( int64_t start, int64_t count ) { return s.post( start, count ); };
		h.jobPoll = [ & ]() { return s.jobPoll(); };
		h.jobWait = [ & ]() { return s.jobWait(); };
		captureLoop::Params lp( cp );
		// a buffer without voice is dropped at dropStartSilence at the latest; the capture buffer holds 30 s and a chunk, so that is where the parameter ends
		lp.dropStartSilence = std::min<uint32_t>( lp.dropStartSilence, (uint32_t)( 30 * captureLoop::SAMPLE_RATE ) );
		captureLoop::Loop loop( lp, h );
		s.loop = &loop;
		return loop.run();
	}
}
