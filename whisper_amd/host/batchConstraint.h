// Constrained decoding on the host ("Constrained decoding"): the checked copy of a caller's automaton together with the vocabulary's bytes,
// as ContextImpl and the lock-step batch runner hold it, and the device half as the scheduler reaches it, the signature of wh_context_set_constraint.
// batchScheduler.cpp holds NO reference to that symbol -- its CPU test library links against a test double of the compute layer that does not have it:
// whisperImpl.cpp installs &wh_context_set_constraint here when libWhisper.so is loaded. nullptr: Whisper::setBatchDecodingConstraint answers E_NOTIMPL.
#pragma once
#include "hostCommon.h"
#include "whisper_hip.h"
#include <cstdint>
#include <vector>

namespace Whisper
{
	using pfnBatchConstraint = int ( * )( wh_context* c, const wh_constraint* k );
	extern pfnBatchConstraint g_batchConstraint;

	// a constraint the caller's pointers no longer back; empty = off. The vocabulary's text tokens are spelled by the model's own strings, byte for byte
	struct HeldConstraint
	{
		std::vector<uint8_t> classOf, accept, tokBytes;
		std::vector<int32_t> trans, tokOffsets;
		wh_constraint k = {};
		bool on() const { return !trans.empty(); }
		void clear() { *this = HeldConstraint{}; }
		// p has passed optionRules::checkConstraint
		void assign( const sDecodingConstraint& p, const Vocabulary& vocab )
		{
			clear();
			classOf.assign( p.classOf, p.classOf + 256 );
			accept.assign( p.accept, p.accept + p.states );
			trans.assign( p.transitions, p.transitions + (size_t)p.states * p.classes );
			tokOffsets.assign( 1, 0 );
			for( int t = 0; t < vocab.token_eot; t++ )
			{
				const char* const s = vocab.string( t );
				if( s ) tokBytes.insert( tokBytes.end(), (const uint8_t*)s, (const uint8_t*)s + vocab.idToToken[ (size_t)t ].size() );
				tokOffsets.push_back( (int32_t)tokBytes.size() );
			}
			tokBytes.push_back( 0 );	// never an empty array
			k.nStates = (int32_t)p.states; k.nClasses = (int32_t)p.classes; k.start = (int32_t)p.start; k.nTokens = vocab.token_eot;
			k.penalty = p.penalty;
		}
		// the pointers are taken at the call: a copied or moved object never hands out another's
		const wh_constraint* device()
		{
			if( !on() ) return nullptr;
			k.classOf = classOf.data(); k.trans = trans.data(); k.accept = accept.data(); k.tokOffsets = tokOffsets.data(); k.tokBytes = tokBytes.data();
			return &k;
		}
	};
}
