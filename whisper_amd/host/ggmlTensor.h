// The tensor records of a ggml model file: the type table, the bytes of a record's payload and the header's f16 field. Host only, no device, no stream state,
// no other header of this library: tests/quant_cpu/driver.cpp compiles it alone.
//
// The third int of a tensor record is a ggml TYPE (not the header's ftype): 0 f32, 1 f16, and the block-quantized 2 q4_0, 3 q4_1, 6 q5_0, 7 q5_1, 8 q8_0, whose
// payload is count / 32 blocks of 18, 20, 22, 24 resp. 34 bytes, packed without padding (a block = 32 consecutive elements along ne[0], so ne[0] % 32 == 0).
// Everything else is refused by name and number: 4 and 5 (q4_2, q4_3: removed from ggml), 9 (q8_1, never stored) and the K-quants from 10 on.
// The header's f16 field is qntvr * 1000 + ftype, ftype 0 f32, 1 f16, 2 q4_0, 3 q4_1, 7 q8_0, 8 q5_0, 9 q5_1; the block layouts above are those of
// quantization version 2 (the older ones differ without saying so), which is checked where a quantized record is met: for a file of f32 and f16 tensors the
// field means nothing to the loader. The reference predates all of this; the device side is wh_dequantize of whisper_hip.h.
#pragma once
#include <cstdint>
#include <string>

namespace Whisper
{
	namespace ggml
	{
		enum eType : int { TYPE_F32 = 0, TYPE_F16 = 1, TYPE_Q4_0 = 2, TYPE_Q4_1 = 3, TYPE_Q5_0 = 6, TYPE_Q5_1 = 7, TYPE_Q8_0 = 8 };
		constexpr int BLOCK_ELEMENTS = 32;
		constexpr int QNT_VERSION = 2;
		constexpr int64_t MAX_BLOCKS = ( (int64_t)1 << 31 ) - 1;	 // what wh_dequantize takes
		constexpr const char* SUPPORTED = "f32, f16, q4_0, q4_1, q5_0, q5_1 and q8_0";

		inline const char* typeName( int type )
		{
			static const char* const names[] = { "f32", "f16", "q4_0", "q4_1", "q4_2 (removed from ggml)", "q4_3 (removed from ggml)", "q5_0", "q5_1", "q8_0", "q8_1",
				"q2_k", "q3_k", "q4_k", "q5_k", "q6_k", "q8_k" };
			return type >= 0 && type < (int)( sizeof( names ) / sizeof( names[ 0 ] ) ) ? names[ type ] : "unknown";
		}
		// bytes of one block of a quantized type; 0 for every other number
		inline int blockBytes( int type )
		{
			switch( type )
			{
			case TYPE_Q4_0: return 18;
			case TYPE_Q4_1: return 20;
			case TYPE_Q5_0: return 22;
			case TYPE_Q5_1: return 24;
			case TYPE_Q8_0: return 34;
			default: return 0;
			}
		}
		inline bool isQuantized( int type ) { return blockBytes( type ) != 0; }
		inline bool isSupported( int type ) { return type == TYPE_F32 || type == TYPE_F16 || isQuantized( type ); }

		// the header's f16 field
		struct FileType { int qntvr, ftype; };
		inline FileType splitFileType( int32_t f16 ) { return FileType{ f16 / 1000, f16 % 1000 }; }
		inline const char* fileTypeName( int ftype )
		{
			switch( ftype )
			{
			case 0: return "f32";
			case 1: return "f16";
			case 2: return "q4_0";
			case 3: return "q4_1";
			case 7: return "q8_0";
			case 8: return "q5_0";
			case 9: return "q5_1";
			default: return "unknown";
			}
		}
		// "q5_0, quantization version 2" / "f16"
		inline std::string describeFileType( int32_t f16 )
		{
			const FileType t = splitFileType( f16 );
			std::string r = fileTypeName( t.ftype );
			if( r == "unknown" ) r += " ftype " + std::to_string( t.ftype );
			if( t.ftype >= 2 || t.qntvr != 0 ) r += ", quantization version " + std::to_string( t.qntvr );
			return r;
		}

		// Payload of one record. true: `count` elements in `bytes` bytes. false: `error` says the type and the reason (the caller adds the tensor's name).
		// Checked: nDims 1 .. 3, ne > 0, the type, a product that fits int64, ne[0] % 32 and the block count for quantized types, the quantization version.
		inline bool payloadBytes( int type, int nDims, const int32_t* ne, int32_t fileF16, int64_t& count, int64_t& bytes, std::string& error )
		{
			count = bytes = 0;
			if( !isSupported( type ) )
			{
				error = "ggml type " + std::to_string( type ) + " (" + typeName( type ) + ") is not supported: " + SUPPORTED + " are";
				return false;
			}
			if( nDims < 1 || nDims > 3 || !ne )
			{
				error = std::string( "type " ) + typeName( type ) + ": " + std::to_string( nDims ) + " dimensions (1 to 3 are valid)";
				return false;
			}
			int64_t n = 1;
			for( int i = 0; i < nDims; i++ )
			{
				if( ne[ i ] <= 0 )
				{
					error = std::string( "type " ) + typeName( type ) + ": dimension " + std::to_string( i ) + " is " + std::to_string( ne[ i ] );
					return false;
				}
				if( n > INT64_MAX / 4 / ne[ i ] )	 // also keeps n * 4 bytes inside int64
				{
					error = std::string( "type " ) + typeName( type ) + ": the element count overflows";
					return false;
				}
				n *= ne[ i ];
			}
			if( !isQuantized( type ) )
			{
				count = n;
				bytes = n * ( type == TYPE_F32 ? 4 : 2 );
				return true;
			}
			const int qntvr = splitFileType( fileF16 ).qntvr;
			if( qntvr != QNT_VERSION )
			{
				error = std::string( "type " ) + typeName( type ) + ": the file's quantization version is " + std::to_string( qntvr ) + ", only the block layouts of version " +
					std::to_string( QNT_VERSION ) + " are read";
				return false;
			}
			if( ( ne[ 0 ] % BLOCK_ELEMENTS ) != 0 )
			{
				error = std::string( "type " ) + typeName( type ) + ": rows of " + std::to_string( ne[ 0 ] ) + " elements are not whole blocks of " + std::to_string( BLOCK_ELEMENTS );
				return false;
			}
			if( n / BLOCK_ELEMENTS > MAX_BLOCKS )
			{
				error = std::string( "type " ) + typeName( type ) + ": " + std::to_string( n / BLOCK_ELEMENTS ) + " blocks, more than 2^31 - 1";
				return false;
			}
			count = n;
			bytes = n / BLOCK_ELEMENTS * blockBytes( type );
			return true;
		}
	}
}
