// RIFF/WAVE header parsing for the iMediaFoundation stand-in: the chunk walk, the `fmt ` chunk (plain and WAVE_FORMAT_EXTENSIBLE), the `data` chunk clipped
// to the file, and the rules for what the decoder accepts. Host only, no device, no other header of this library: tests/wav_cpu/driver.cpp compiles it alone.
//
// Accepted: integer PCM of 8 (unsigned), 16, 24 and 32 bits and IEEE float32, 1 .. 8 interleaved channels, 1000 .. 384000 Hz. What the reference gets from
// the OS for any container and codec (Whisper/MF/loadAudioFile.cpp) is limited to this here: decoding codecs needs Media Foundation, converting the
// rate, the bit depth and the channel count of plain PCM does not (whisper_hip.h: wh_resample).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

namespace Whisper
{
	namespace wav
	{
		// the values of wh_pcm_format (whisper_hip.h)
		enum ePcmFormat : int { PCM_U8 = 0, PCM_S16 = 1, PCM_S24 = 2, PCM_S32 = 3, PCM_F32 = 4 };
		constexpr int MIN_RATE = 1000, MAX_RATE = 384000, MAX_CHANNELS = 8;
		constexpr const char* ACCEPTED = "RIFF/WAVE with PCM of 8, 16, 24 or 32 bits or float32, 1 to 8 channels, 1000 to 384000 Hz";

		struct Info
		{
			int format = 0;			 // ePcmFormat
			int channels = 0;
			int rate = 0;
			size_t firstByte = 0;	 // offset of the first sample in the file
			size_t frames = 0;		 // whole frames the file holds (a `data` length beyond the end of the file is clipped to it)
		};
		inline int bytesPerSample( int format ) { return format == PCM_U8 ? 1 : format == PCM_S16 ? 2 : format == PCM_S24 ? 3 : 4; }

		inline uint16_t rd16( const uint8_t* p ) { return (uint16_t)( p[ 0 ] | ( p[ 1 ] << 8 ) ); }
		inline uint32_t rd32( const uint8_t* p ) { return (uint32_t)p[ 0 ] | ( (uint32_t)p[ 1 ] << 8 ) | ( (uint32_t)p[ 2 ] << 16 ) | ( (uint32_t)p[ 3 ] << 24 ); }

		// true and `info`, or false and a text that says what is wrong and what is accepted
		inline bool parse( const void* data, size_t size, Info& info, std::string& error )
		{
			const uint8_t* const bytes = (const uint8_t*)data;
			if( !bytes || size < 12 || memcmp( bytes, "RIFF", 4 ) || memcmp( bytes + 8, "WAVE", 4 ) )
			{
				error = "not a RIFF/WAVE file (only WAV is supported on this platform)";
				return false;
			}
			bool haveFmt = false, haveData = false;
			uint32_t tag = 0, channels = 0, rate = 0, blockAlign = 0, bits = 0;
			size_t dataAt = 0, dataBytes = 0;
			for( size_t o = 12; o + 8 <= size; )
			{
				const uint32_t len = rd32( bytes + o + 4 );
				const size_t body = o + 8, avail = size - body;
				if( !memcmp( bytes + o, "fmt ", 4 ) )
				{
					if( len < 16 || avail < 16 ) { error = "the fmt chunk is truncated"; return false; }
					const uint8_t* f = bytes + body;
					tag = rd16( f ); channels = rd16( f + 2 ); rate = rd32( f + 4 ); blockAlign = rd16( f + 12 ); bits = rd16( f + 14 );
					if( tag == 0xFFFE )
					{
						// WAVEFORMATEXTENSIBLE: cbSize 22 = valid bits, channel mask, sub-format GUID whose first two bytes are the plain format tag and
						// whose other 14 are fixed (KSDATAFORMAT_SUBTYPE_PCM / _IEEE_FLOAT)
						static const uint8_t guidTail[ 14 ] = { 0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71 };
						if( len < 40 || avail < 40 || rd16( f + 16 ) < 22 ) { error = "the extensible fmt chunk is truncated"; return false; }
						if( memcmp( f + 26, guidTail, 14 ) ) { error = "the extensible sub-format is not PCM or IEEE float"; return false; }
						tag = rd16( f + 24 );
					}
					haveFmt = true;
				}
				else if( !memcmp( bytes + o, "data", 4 ) )
				{
					dataAt = body;
					dataBytes = (size_t)len < avail ? (size_t)len : avail;
					haveData = true;
				}
				if( (size_t)len >= avail ) break;	  // the chunk reaches the end of the file
				o = body + (size_t)len + ( len & 1 );	  // chunks are padded to even lengths
			}
			if( !haveFmt ) { error = "no fmt chunk"; return false; }
			if( !haveData ) { error = "no data chunk"; return false; }
			int format = -1;
			if( tag == 1 ) format = bits == 8 ? PCM_U8 : bits == 16 ? PCM_S16 : bits == 24 ? PCM_S24 : bits == 32 ? PCM_S32 : -1;
			else if( tag == 3 && bits == 32 ) format = PCM_F32;
			char got[ 160 ];
			snprintf( got, sizeof( got ), " (got format %u, %u bit, %u ch, %u Hz, block of %u bytes)", tag, bits, channels, rate, blockAlign );
			if( format < 0 || channels < 1 || channels > (uint32_t)MAX_CHANNELS || rate < (uint32_t)MIN_RATE || rate > (uint32_t)MAX_RATE )
			{
				error = std::string( "need " ) + ACCEPTED + got;
				return false;
			}
			if( blockAlign != channels * (uint32_t)bytesPerSample( format ) )
			{
				error = std::string( "the block size is not channels x bytes per sample; need " ) + ACCEPTED + got;
				return false;
			}
			info.format = format;
			info.channels = (int)channels;
			info.rate = (int)rate;
			info.firstByte = dataAt;
			info.frames = dataBytes / blockAlign;
			return true;
		}

		// one sample as a float: u8 ( v - 128 ) / 128, s16 v / 32768, s24 v / 8388608, s32 (float)( v * 2^-31 ) from double, f32 as is
		inline float sample( const uint8_t* p, int format )
		{
			switch( format )
			{
			case PCM_U8: return (float)( (int)p[ 0 ] - 128 ) / 128.0f;
			case PCM_S16: return (float)(int16_t)rd16( p ) / 32768.0f;
			case PCM_S24: return (float)( (int32_t)( ( (uint32_t)p[ 0 ] << 8 ) | ( (uint32_t)p[ 1 ] << 16 ) | ( (uint32_t)p[ 2 ] << 24 ) ) >> 8 ) / 8388608.0f;
			case PCM_S32: return (float)( (double)(int32_t)rd32( p ) * ( 1.0 / 2147483648.0 ) );
			default: { float v; memcpy( &v, p, 4 ); return v; }
			}
		}
	}
}
